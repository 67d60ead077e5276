// realign_walk_kernel.h — alignment::realign scored by a FIXED-BLOCK WALK over the affine-gap matrix instead of the exact DP of realign_kernel.h:
// the family scripts/probes/block_walk.c defines (walk_score) and scripts/block_walk_family.py measured.  A block of 8 x 8 cells (plus its border
// row / column: 9 x 9) starts at the top-left corner of the 33 x 33 matrix and is shifted right or down by STEP cells until it holds cell (32, 32);
// the direction compares the block's right border column with its bottom border row (RULE 0: maxima, 1: sums; TIE 0: right, 1: down); a cell whose
// neighbour was never computed sees -infinity from it.  Same argument block (RealignArgs), windows, scores (NW1, open -2, extend -1), outputs and first-best rule as realign_kernel.h.
// No member of the family is known to be block-aligner's walk (the crate is not available): the members are selectable, none is pinned.
//
// What a later block can still read.  The block's origin only grows, so the cells a shift reads are (a) the current block's border in the direction
// of the move, i.e. for every row of the block the RIGHTMOST cell computed so far (shift right) or for every column the LOWEST one (shift down),
// and (b) one corner cell diagonally outside the block, which was computed iff the previous shift was perpendicular to this one (then the block it
// left behind covers that cell; after a parallel shift, or at the start, no block ever reached it).  The new strip's other outer neighbours lie
// beyond every earlier block and are never computed.  So the state of an alignment is two arrays of 33 entries, row[i] = (best, gap-in-row) of the
// rightmost cell of row i and col[j] = (best, gap-in-column) of the lowest cell of column j: 264 bytes of LDS instead of the 6.5 KB matrix, and
// no `done` flags.  The borders the direction rule compares are row[i0 .. i0 + 8] and col[j0 .. j0 + 8].  With 32 x 32 windows, block 8 and a step
// that divides 24 the walk never clamps and always takes 24 / STEP shifts each way: the loop count is uniform, only the order is data.
//
// Mapping.  One 16-lane group (a DPP row) per window, the alleles one after the other; 4 windows per wavefront, 16 per workgroup.  A shift computes a
// strip of 9 x STEP cells as a systolic array, the same scheme as realign_kernel.h: lane p (0 .. 8) owns position p across the move (a row for a
// shift right, a column for a shift down) and computes cell k = t - p along the move at step t; the cell behind it is its own previous value, the
// cell across arrives from lane p - 1 with one DPP row shift per state, the diagonal is what arrived one step earlier.  The two directions are the
// same code with the roles of the sequences and of the two gap states exchanged, so groups that go different ways do not diverge.  The first block
// is a shift right by 8 from column 0.  Integer arithmetic, bit-equal to walk_score (tests/test_gpu_realign_walk.py).
#pragma once
#include "realign_kernel.h"

namespace fl {

namespace walk {
constexpr int W = 32, FLANK = 16, B = 8, OPEN = -2, EXTEND = -1, NEG = -16384;      // NEG: far below any score (>= -100), fits the 16-bit halves below
constexpr int PAD = 40;                                                              // row[] / col[] entries: 33 used, lanes 9 .. 15 of a group read up to 24 + 15
constexpr int GROUPS = 16;                                                           // windows per workgroup of 256 lanes
__device__ __forceinline__ uint32_t pack(int best, int gap) { return ((uint32_t)best & 0xffffu) | ((uint32_t)gap << 16); }
__device__ __forceinline__ int lo16(uint32_t v) { return (int)(v << 16) >> 16; }
__device__ __forceinline__ int hi16(uint32_t v) { return (int)v >> 16; }
__device__ __forceinline__ int max2(int a, int b) { return a > b ? a : b; }
template <int N> __device__ __forceinline__ int ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, false); }   // row_ror:N, within 16 lanes
__device__ __forceinline__ int shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); }                      // row_shr:1

struct Lds {
    uint32_t row[GROUPS][PAD], col[GROUPS][PAD];      // (best | gap << 16) of the rightmost cell of a row / the lowest cell of a column
    uint8_t q[GROUPS][W], r[GROUPS][W];
};

// One shift of S cells.  `from` holds the border the strip grows out of (row[] for a shift right), `to` receives the far end of every new line
// (col[] for a shift right); `fixed` is the sequence along the block's edge (the read for a shift right), `moving` the one the strip consumes.
// origin = the block's first row (right) / column (down), edge = its last column (right) / row (down), corner = the diagonal cell outside exists.
template <int S> __device__ __forceinline__ void strip(uint32_t* from, uint32_t* to, const uint8_t* fixed, const uint8_t* moving, int p, int origin, int edge, bool corner) {
    const int idx = origin + p;                                   // absolute row (right) / column (down) of this lane's line
    const uint32_t w0 = from[idx], wd = from[idx > 0 ? idx - 1 : 0];
    int best = lo16(w0), along = hi16(w0), across = NEG;          // the line's last computed cell: best, the gap state along the move; across = this lane's newest gap state across it
    int diag = (idx > 0 && (p > 0 || corner)) ? lo16(wd) : NEG;
    const int fb = fixed[(idx - 1) & (W - 1)];                     // (row / column 0 has no base, and lanes 9 .. 15 compute nothing: any in-range byte)
#pragma unroll
    for (int t = 0; t < S + B; ++t) {
        const int k = t - p;
        const bool active = p <= B && k >= 0 && k < S;
        int xb = shr1(best), xg = shr1(across);                   // lane p - 1 computed its cell k in the previous step
        if (p == 0) { xb = NEG; xg = NEG; }
        const int mb = moving[(edge + k) & (W - 1)];              // cell edge + 1 + k consumes base edge + k
        const int sub = (idx > 0 && fb == mb) ? 1 : -1;
        const int na = max2(max2(best + OPEN, along + EXTEND), NEG);
        const int nx = max2(max2(xb + OPEN, xg + EXTEND), NEG);
        const int nb = max2(max2(diag + sub, na), max2(nx, NEG));
        if (active) {
            best = nb; along = na; across = nx; diag = xb;
            if (p == B) to[edge + 1 + k] = pack(nb, nx);
        }
    }
    if (p <= B) from[idx] = pack(best, along);
}

__device__ __forceinline__ int row_sum(int v) { v += ror<8>(v); v += ror<4>(v); v += ror<2>(v); v += ror<1>(v); return v; }
__device__ __forceinline__ int row_max(int v) { v = max2(v, ror<8>(v)); v = max2(v, ror<4>(v)); v = max2(v, ror<2>(v)); v = max2(v, ror<1>(v)); return v; }
}  // namespace walk

template <int STEP, int RULE, int TIE> __global__ __launch_bounds__(256) void realign_walk_kernel(RealignArgs g) {
    using namespace walk;
    static_assert((W - B) % STEP == 0 && STEP >= 1 && STEP <= B, "the walk must reach the far corner without clamping");
    __shared__ Lds lds;
    const int p = (int)(threadIdx.x & 15);
    const uint32_t grp = threadIdx.x >> 4;
    uint32_t* const row = lds.row[grp];
    uint32_t* const col = lds.col[grp];
    uint8_t* const lq = lds.q[grp];
    uint8_t* const lr = lds.r[grp];
    const uint64_t stride = (uint64_t)gridDim.x * GROUPS;
    // every group of a wavefront runs the same number of rounds (the DPP row operations want whole rows, the loop stays uniform); a group past the
    // end scores window n - 1 again and stores nothing
    const uint64_t rounds = (g.n + stride - 1) / stride;
    for (uint64_t it = 0; it < rounds; ++it) {
        const uint64_t w_raw = it * stride + (uint64_t)blockIdx.x * GROUPS + grp;
        const bool live = w_raw < g.n;
        const uint64_t w = live ? w_raw : g.n - 1;
        lq[p] = g.q[w * W + p]; lq[p + 16] = g.q[w * W + p + 16];
        lr[p] = g.r[w * W + p]; lr[p + 16] = g.r[w * W + p + 16];
        const uint32_t na = g.n_alleles[w];
        int best_score = INT32_MIN;
        uint32_t best = 0;
        for (uint32_t a = 0; a < FLORIA_MAX_ALLELES; ++a) {
            // groups with fewer alleles score their last one again; the loop ends when no group of the wavefront has one left
            if (__builtin_amdgcn_ballot_w64(a < na) == 0) break;
            const uint32_t ax = a < na ? a : na - 1;
            if (p == 0) lr[FLANK] = g.alleles[w * FLORIA_MAX_ALLELES + ax];
            // column 0: best(i, 0) = gap-in-column(i, 0) = open + (i - 1) extend, no gap-in-row state; then the first block as a shift right by 8
            if (p <= B) row[p] = pack(p == 0 ? 0 : OPEN + (p - 1) * EXTEND, NEG);
            if (p == 0) col[0] = pack(OPEN + (B - 1) * EXTEND, OPEN + (B - 1) * EXTEND);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            strip<B>(row, col, lq, lr, p, 0, 0, false);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            int i0 = 0, j0 = 0, last = -1;                         // last: direction of the previous shift (0 right, 1 down)
#pragma unroll 1
            for (int mv = 0; mv < 2 * (W - B) / STEP; ++mv) {
                // right border = row[i0 .. i0 + 8], bottom border = col[j0 .. j0 + 8]; reduced in every group (whole DPP rows), used away from the edges
                const int rb = p <= B ? lo16(row[i0 + p]) : (RULE ? 0 : NEG), cb = p <= B ? lo16(col[j0 + p]) : (RULE ? 0 : NEG);
                int dir;
                if (RULE) { const int d = row_sum(cb - rb); dir = d > 0 ? 1 : (d < 0 ? 0 : TIE); }
                else { const int ra = row_max(rb), ca = row_max(cb); dir = ca > ra ? 1 : (ra > ca ? 0 : TIE); }
                if (j0 + B == W) dir = 1; else if (i0 + B == W) dir = 0;
                const bool down = dir != 0;
                strip<STEP>(down ? col : row, down ? row : col, down ? lr : lq, down ? lq : lr, p, down ? j0 : i0, (down ? i0 : j0) + B, last == (dir ^ 1));
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (down) i0 += STEP; else j0 += STEP;
                last = dir;
            }
            const int s = lo16(row[W]);                            // cell (32, 32)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (a < na && s > best_score) { best_score = s; best = a; }
        }
        if (live && p == 0) { g.best[w] = (uint8_t)best; if (g.score) g.score[w] = best_score; }
    }
}

}  // namespace fl
