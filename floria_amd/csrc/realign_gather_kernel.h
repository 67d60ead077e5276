// realign_gather_kernel.h — alignment::realign (alignment.rs:7-64) for the cells of floria_hip_pileup_records while they are still on the device
// (floria_hip_pileup_records_realign): the two 32-byte windows of a call are cut from bytes that are already in HBM — the read's 4-bit bases in the
// uploaded record blob, the contig's reference sequence — the exact shortcut decides what it can, and what it cannot goes to realign_kernel /
// realign_walk_kernel<..> unchanged, as a work list of windows in their layout (fl::RealignArgs).
//
// A 32-lane half of a wavefront per cell, lane = window column (grid-stride over the cells, 8 cells per workgroup and trip):
//   * the cell's record is the last one whose cell_off is <= the cell (a binary search, the same addresses in all 32 lanes of a half);
//   * bounds (alignment.rs:21-27, in 64 bits): 16 <= G, G + 16 < R, 16 <= p, p + 16 < L with G the SNP's position, R the length of the contig's reference
//     (0 = the contig has none), p the cell's seq_pos (hard-clip shift included, as the host route uses it) and L the record's l_seq.  A cell outside keeps
//     its allele and no byte of a window is read for it;
//   * q[j] = base p - 16 + j of the record (anything but A C G T becomes A), r[j] = the upper-cased reference byte G - 16 + j; h = mismatches outside
//     column 16: one ballot, a popcount per half;
//   * h <= 2 and an allele equal to q[16]: the first such; else h <= 1: allele 0; else the cell is undecided.
// DECIDE (first pass) stores the decided alleles, flags the undecided cells (one byte per cell) and counts; the host reads the count and sizes the work list from it.
// FILL (second pass) visits the flagged cells only and appends their windows: one atomic per wavefront for the slots (ballot + the rank of the half), so the list's
// order is whatever the hardware makes it — every entry carries its cell, and realign_scatter_kernel stores best[] by that.
// Every index is bounded by what the host validated (floria_hip.hip: pileup_validate, refs_validate) and by the bounds rule itself: p + 15 < l_seq lies inside the
// record's sequence bytes, G + 15 < R inside the contig's reference.  No LDS, no scratch.
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

struct RealignGatherArgs {
    const uint8_t*  blob;
    const uint32_t* contig;     // [n_records]
    const uint64_t* seq_off;    // [n_records]
    const uint32_t* l_seq;      // [n_records]
    const uint64_t* cell_off;   // [n_records + 1] exclusive offsets
    const uint64_t* snp_off;    // [n_contigs + 1]
    const int64_t*  snp_pos;    // indexed with the caller's offsets, as in PileupArgs
    const uint8_t*  alleles;
    const uint8_t*  n_alleles;
    const uint64_t* ref_off;    // [n_contigs + 1]
    const uint8_t*  ref_seq;
    const uint32_t* snp;        // [n_cells] rank in the contig + 1
    const uint32_t* seq_pos;    // [n_cells]
    uint8_t*  allele;           // [n_cells] in: as walked; out: realigned
    uint8_t*  undecided;        // [n_cells] DECIDE: 1 = goes to the scoring kernel
    uint64_t* counts;           // [RG_N_COUNTS]
    uint8_t*  wq;               // FILL outputs: [cap][32], [cap][32], [cap][FLORIA_MAX_ALLELES], [cap], [cap]
    uint8_t*  wr;
    uint8_t*  wal;
    uint8_t*  wna;
    uint64_t* wcell;
    uint64_t  cap;              // entries the work list holds (= counts[RG_SCORED] after DECIDE)
    uint64_t  n_cells;
    uint32_t  n_records;
};
enum { RG_IN_BOUNDS = 0, RG_SHORTCUT = 1, RG_SCORED = 2, RG_CHANGED = 3, RG_APPENDED = 4, RG_N_COUNTS = 8 };

__device__ __forceinline__ uint32_t rg_upper(uint32_t c) { return (c >= 'a' && c <= 'z') ? c - 32u : c; }

// the windows of one cell, column `col` in this lane; false: outside the bounds (nothing was read)
struct RealignCell { uint32_t q, r, al, na; };
__device__ __forceinline__ bool realign_gather_cell(const RealignGatherArgs& g, uint64_t cell, uint32_t col, RealignCell& w) {
    constexpr uint64_t NT16_LO = 0x565352474d43413dull, NT16_HI = 0x4e42444b48595754ull;      // "=ACMGRSV", "TWYHKDBN": the base of a 4-bit code
    uint32_t lo = 0, hi = g.n_records;                   // cell_off[lo] <= cell < cell_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (g.cell_off[mid] <= cell) lo = mid; else hi = mid;
    }
    const uint32_t c = g.contig[lo];
    const uint64_t k = g.snp_off[c] + (g.snp[cell] - 1u);
    const int64_t G = g.snp_pos[k];
    const uint64_t p = g.seq_pos[cell], L = g.l_seq[lo], r0 = g.ref_off[c], R = g.ref_off[c + 1] - r0;
    if (!(G >= 16 && (uint64_t)G + 16 < R && p >= 16 && p + 16 < L)) return false;
    const uint64_t sp = p - 16 + col;
    const uint32_t byte = g.blob[g.seq_off[lo] + (sp >> 1)], code = (sp & 1) ? (byte & 15u) : (byte >> 4);
    const uint32_t base = (uint32_t)(((code & 8u) ? NT16_HI : NT16_LO) >> (8 * (code & 7u))) & 0xffu;
    w.q = (base == 'A' || base == 'C' || base == 'G' || base == 'T') ? base : (uint32_t)'A';
    w.r = rg_upper(g.ref_seq[r0 + ((uint64_t)G - 16 + col)]);
    const uint32_t al = *(const uint32_t*)(g.alleles + 4 * k);
    w.al = rg_upper(al & 0xffu) | rg_upper((al >> 8) & 0xffu) << 8 | rg_upper((al >> 16) & 0xffu) << 16 | rg_upper(al >> 24) << 24;
    w.na = g.n_alleles[k];
    return true;
}

__global__ __launch_bounds__(256) void realign_decide_kernel(RealignGatherArgs g) {
    const uint32_t lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * 8;
    uint32_t n_in = 0, n_short = 0, n_und = 0, n_changed = 0;          // this lane's cells (column 0 of a half counts)
    for (uint64_t cell = (uint64_t)blockIdx.x * 8 + (threadIdx.x >> 5); cell < g.n_cells; cell += stride) {
        RealignCell w{};
        const bool in = realign_gather_cell(g, cell, col, w);
        const uint64_t mm = __ballot(in && col != 16 && w.q != w.r);
        if (!in) { if (col == 0) g.undecided[cell] = 0; continue; }
        const uint32_t h = (uint32_t)__popc((uint32_t)(mm >> (32 * half)));
        const uint32_t q16 = (uint32_t)__shfl((int)w.q, (int)((lane & 32u) | 16u), 64);
        uint32_t m = w.na;
#pragma unroll
        for (uint32_t t = 4; t-- > 0;) if (t < w.na && ((w.al >> (8 * t)) & 0xffu) == q16) m = t;      // the first allele equal to the read's base
        const bool by_base = h <= 2 && m < w.na, by_first = !by_base && h <= 1, und = !by_base && !by_first;
        if (col == 0) {
            g.undecided[cell] = und ? 1 : 0;
            ++n_in;
            if (und) ++n_und;
            else {
                const uint8_t a = (uint8_t)(by_base ? m : 0u);
                ++n_short;
                if (g.allele[cell] != a) { ++n_changed; g.allele[cell] = a; }
            }
        }
    }
    // one add per wavefront and counter: the two column-0 lanes hold the wave's numbers
    const uint32_t a = n_in + (uint32_t)__shfl((int)n_in, 32, 64), b = n_short + (uint32_t)__shfl((int)n_short, 32, 64);
    const uint32_t c = n_und + (uint32_t)__shfl((int)n_und, 32, 64), d = n_changed + (uint32_t)__shfl((int)n_changed, 32, 64);
    if (lane == 0) {
        if (a) atomicAdd((unsigned long long*)&g.counts[RG_IN_BOUNDS], (unsigned long long)a);
        if (b) atomicAdd((unsigned long long*)&g.counts[RG_SHORTCUT], (unsigned long long)b);
        if (c) atomicAdd((unsigned long long*)&g.counts[RG_SCORED], (unsigned long long)c);
        if (d) atomicAdd((unsigned long long*)&g.counts[RG_CHANGED], (unsigned long long)d);
    }
}

__global__ __launch_bounds__(256) void realign_fill_kernel(RealignGatherArgs g) {
    const uint32_t lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * 8;
    for (uint64_t cell = (uint64_t)blockIdx.x * 8 + (threadIdx.x >> 5); cell < g.n_cells; cell += stride) {
        RealignCell w{};
        const bool und = g.undecided[cell] != 0 && realign_gather_cell(g, cell, col, w);      // (a flagged cell is inside the bounds)
        const uint64_t um = __ballot(und && col == 0);                                         // bit 0 / bit 32: the halves that append
        if (um == 0) continue;
        uint64_t base = 0;
        if (lane == 0) base = atomicAdd((unsigned long long*)&g.counts[RG_APPENDED], (unsigned long long)__popcll(um));
        base = rl64(base, 0);
        const uint64_t slot = base + (half ? (uint32_t)(um & 1u) : 0u);
        if (und && slot < g.cap) {
            g.wq[32 * slot + col] = (uint8_t)w.q;
            g.wr[32 * slot + col] = (uint8_t)w.r;
            if (col < 4) g.wal[4 * slot + col] = col < w.na ? (uint8_t)(w.al >> (8 * col)) : (uint8_t)0;
            if (col == 0) { g.wna[slot] = (uint8_t)w.na; g.wcell[slot] = cell; }
        }
    }
}

// best[i] of the scoring kernel -> the allele of the cell entry i came from
__global__ __launch_bounds__(256) void realign_scatter_kernel(const uint8_t* best, const uint64_t* wcell, uint64_t n, uint8_t* allele, uint64_t* counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint32_t n_changed = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t cell = wcell[i];
        const uint8_t b = best[i];
        if (allele[cell] != b) { ++n_changed; allele[cell] = b; }
    }
    const uint64_t any = __ballot(n_changed != 0);
    if (any) {
#pragma unroll
        for (uint32_t d = 32; d > 0; d >>= 1) n_changed += (uint32_t)__shfl_xor((int)n_changed, (int)d, 64);
        if (lane == 0) atomicAdd((unsigned long long*)&counts[RG_CHANGED], (unsigned long long)n_changed);
    }
}

}  // namespace fl
