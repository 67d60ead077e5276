// assemble_order_kernel.h — Frag.positions of the fragments floria_hip_assemble_contigs merged (floria_hip_assemble_contigs_ordered): for every fragment of a
// contig that holds a merged fragment, the iteration order of the reference's FxHashSet of SNP positions, as floria_pileup::set_order states it, derived on the
// device from what assemble_kernel<FILL> left there.  For the parts p0, p1, .. of a fragment in list order (combine_frags, file_reader.rs:539-541, 636-639):
//   * a part's own set: an empty map receives the part's SNPs ascending, growing as it goes (the CIGAR walk's seq_dict); an empty set reserves room for all of
//     them at once and receives the map's keys in bucket order (`keys().collect()`).  A part without cells leaves the unallocated empty set;
//   * the accumulator starts as p0's set.  Every later part: reserve(acc empty ? n : (n + 1) / 2), then `insert` of the part's keys in the iteration order of the
//     part's own set (`positions.extend(other.positions)`); insert reserves room for one key before it looks the key up (FxTable::insert);
//   * set_order[first merged cell + j] = the place in the fragment's ascending merged SNP list of the j-th key in the accumulator's bucket order.
// Two kernels in the manner of cell_order_direct_kernel / cell_order_kernel (arith_kernel.h):
//   assemble_order_kernel          a WAVEFRONT per fragment, five tables of AO_NB buckets in LDS (the accumulator and its spare, the growing map and its spare, the
//                                  part's set); a probe group is one ballot (FxWave).  It takes the fragments whose parts have at most AO_FAST_CELLS cells together —
//                                  no table of such a fragment outgrows AO_NB buckets — and lists the others.  A part whose SNPs span fewer positions than its set
//                                  has buckets needs no map: bucket b of the set holds the one position of the span that is congruent to b * K^-1 (the home-bucket rule);
//   assemble_order_general_kernel  a THREAD per listed fragment, five FxTables in global scratch sized by the host for the largest sum of parts' cells.
// Whatever does not add up on the device (a sum of cells beyond the scratch, an accumulator that does not end with the fragment's merged cells, a key that is not
// in the merged list) leaves the fragment's entries as the host preset them (all ones) or writes all ones: the permutation check of the cell orders that run next
// (cell_order_direct_kernel) then refuses the call.  No index reaches memory before it was compared with a length: the records and parts with the counts the host
// validated, the parts' cells with the table size, the output with the fragment's merged cells.
#pragma once
#include "arith_kernel.h"
#include "assemble_kernel.h"

namespace fl {

constexpr uint32_t AO_FAST_CELLS = 223;      // fx_buckets_for(223 + 1) = 256: the largest sum of parts' cells whose every table (reserve(1) on a full one included) stays within AO_NB buckets
constexpr uint32_t AO_NB = 256;
constexpr uint32_t AO_CTRL = AO_NB + FX_W + 16;      // fx_ctrl_bytes(224)
constexpr uint32_t AO_TABLES = 5;            // 5 * (288 + 1024) B = 6 560 B per wavefront, 26 240 B per workgroup: six workgroups per CU by LDS
constexpr uint32_t AO_NONE = 0xffffffffu;

struct AsmOrderArgs {
    // the resident pileup
    const uint64_t* cell_off;     // [n_records + 1]
    const uint32_t* snp;
    // the fragment plan, as AssembleArgs has it, and FILL's outputs
    const uint64_t* part_off;     // [n_frags + 1]
    const uint32_t* part_rec;     // [n_parts]
    const uint32_t* frag_ctg;     // [n_frags]
    const uint64_t* frag_cells;   // [n_frags + 1] exclusive offsets of the merged cells
    const uint32_t* merged_snp;   // [total_cells] the arena's raw SNP region
    const uint32_t* ctg_merged;   // [n_contigs] != 0: the contig carries a set_order
    uint32_t* set_order;          // [total_cells] (out) the arena's set-order region, preset to all ones
    uint64_t* todo;               // [1 + n_frags] number of fragments left to the general kernel, then their indices
    uint64_t  n_frags, n_parts, total_cells;
    uint32_t  n_records, n_contigs;
    uint32_t  force_general;      // (tests) != 0: every fragment goes the long way
    // the general kernel
    uint8_t*  scratch;            // [n_threads][AO_TABLES * (ctrl_bytes + slot_bytes)]
    uint64_t  scratch_bytes, ctrl_bytes, slot_bytes;
    uint32_t  cells_max;          // the largest sum of parts' cells the tables were sized for
    uint32_t  n_threads;
};

__device__ __forceinline__ uint64_t asm_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32) | __shfl_xor((uint32_t)v, o);
    return v;
}

// the place of `key` in the ascending list m[0, M), AO_NONE if it is not there
__device__ __forceinline__ uint32_t asm_order_index(const uint32_t* m, uint32_t M, uint32_t key) {
    uint32_t a = 0, b = M;
    while (a < b) { const uint32_t mid = (a + b) >> 1; if (m[mid] < key) a = mid + 1; else b = mid; }
    return a < M && m[a] == key ? a : AO_NONE;
}

// what both kernels read of a fragment before they touch a table; false = not a fragment of a contig with a set_order, or one whose numbers do not fit their arrays
struct AsmOrderFrag { uint64_t p0, p1, out0; uint32_t M; };
__device__ __forceinline__ bool asm_order_frag(const AsmOrderArgs& g, uint64_t f, AsmOrderFrag& F) {
    const uint32_t ctg = g.frag_ctg[f];
    if (ctg >= g.n_contigs || !g.ctg_merged[ctg]) return false;
    F.p0 = g.part_off[f]; F.p1 = g.part_off[f + 1];
    const uint64_t out1 = g.frag_cells[f + 1];
    F.out0 = g.frag_cells[f];
    if (F.p1 > g.n_parts || F.p1 <= F.p0 || out1 <= F.out0 || out1 > g.total_cells || out1 - F.out0 >= 0xffffffffull) return false;
    F.M = (uint32_t)(out1 - F.out0);
    return true;
}
// the cells [b, b + n) of part p (n = 0: none, or a record index beyond the residency)
__device__ __forceinline__ uint32_t asm_order_part(const AsmOrderArgs& g, uint64_t p, uint64_t& b) {
    const uint32_t rec = g.part_rec[p];
    if (rec >= g.n_records) return 0;
    b = g.cell_off[rec];
    const uint64_t e = g.cell_off[rec + 1];
    return e > b && e - b < 0xffffffffull ? (uint32_t)(e - b) : 0u;
}

__global__ __launch_bounds__(256) void assemble_order_kernel(AsmOrderArgs g) {
    __shared__ __attribute__((aligned(16))) uint8_t s_ctrl[4][AO_TABLES][AO_CTRL];
    __shared__ uint32_t s_slot[4][AO_TABLES][AO_NB];
    const uint32_t lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    uint8_t (*const tc)[AO_CTRL] = s_ctrl[wv];
    uint32_t (*const ts)[AO_NB] = s_slot[wv];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t f = (uint64_t)blockIdx.x * 4 + wv; f < g.n_frags; f += n_waves) {
        AsmOrderFrag F;
        if (!asm_order_frag(g, f, F)) continue;
        uint64_t sum = 0;                                   // the parts' cells together (lanes over the parts)
        for (uint64_t p = F.p0 + lane; p < F.p1; p += 64) { uint64_t b; sum += asm_order_part(g, p, b); }
        sum = asm_wave_sum(sum);
        if (sum > AO_FAST_CELLS || g.force_general) {       // (wave-uniform)
            if (lane == 0) g.todo[1 + atomicAdd((unsigned long long*)g.todo, 1ull)] = f;
            continue;
        }
        if (F.M > sum) continue;
        // (a wavefront's LDS operations execute in order; the fences keep the compiler from moving them across each other)
        FxWave acc;                                         // tables 0 and 1
        uint8_t* acc_sc = tc[1]; uint32_t* acc_ss = ts[1];
        for (uint64_t p = F.p0; p < F.p1; ++p) {
            uint64_t b = 0;
            const uint32_t n = uni(asm_order_part(g, p, b));               // <= sum <= AO_FAST_CELLS
            if (n == 0) continue;
            const uint32_t* ps = g.snp + b;
            const uint32_t first = uni(ps[0]), range = uni(ps[n - 1]) - first, C = fx_buckets_for(n);
            const bool base = p == F.p0, home = range < C;
            if (!base) {
                if (acc.buckets == 0) acc.bind(tc[0], ts[0], C, lane);        // reserve(n) of the unallocated empty set
                else acc.reserve((n + 1) / 2, acc_sc, acc_ss, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            if (home && base) {
                // every key finds its home bucket empty, in whatever order the map hands the keys over
                acc.bind(tc[0], ts[0], C, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (uint32_t c = 0; c < n; ++c) acc.put(uni(ps[c]), lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            } else if (home) {
                uint32_t* const idx = ts[4];                               // position -> is one of the part's (C <= AO_NB entries)
                for (uint32_t x = lane; x <= range; x += 64) idx[x] = 0;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (uint32_t c = lane; c < n; c += 64) { const uint32_t d = ps[c] - first; if (d <= range) idx[d] = 1; }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (uint32_t b0 = 0; b0 < C; b0 += 64) {
                    const uint32_t bk = b0 + lane;
                    const uint32_t off = (bk * FX_KINV32 - first) & (C - 1u);      // the one position of [first, first + C) whose home is bucket bk
                    const bool have = bk < C && off <= range && idx[off] != 0u;
                    uint64_t m = __ballot(have);
                    while (m) {                                            // the part's set in bucket order
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        acc.insert((uint32_t)__shfl((int)(first + off), l), acc_sc, acc_ss, lane);
                    }
                }
            } else {
                FxWave seq;                                                // tables 2 and 3: the growing map
                uint8_t* seq_sc = tc[3]; uint32_t* seq_ss = ts[3];
                seq.bind(tc[2], ts[2], fx_buckets_for(1), lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (uint32_t c = 0; c < n; ++c) seq.insert_new(uni(ps[c]), seq_sc, seq_ss, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                FxWave set;                                                // the part's set: the accumulator itself for the base part, else table 4
                set.bind(base ? tc[0] : tc[4], base ? ts[0] : ts[4], C, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (uint32_t i0 = 0; i0 < seq.buckets; i0 += 64) {
                    const bool in = i0 + lane < seq.buckets;
                    const uint32_t c = in ? seq.ctrl[i0 + lane] : 0xffu;
                    const uint32_t key = in ? seq.slot[i0 + lane] : 0u;
                    uint64_t m = __ballot(!(c & 0x80u));
                    while (m) { const int l = __builtin_ctzll(m); m &= m - 1; set.put((uint32_t)__shfl((int)key, l), lane); }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (base) acc = set;
                else for (uint32_t i0 = 0; i0 < set.buckets; i0 += 64) {
                    const bool in = i0 + lane < set.buckets;
                    const uint32_t c = in ? set.ctrl[i0 + lane] : 0xffu;
                    const uint32_t key = in ? set.slot[i0 + lane] : 0u;
                    uint64_t m = __ballot(!(c & 0x80u));
                    while (m) { const int l = __builtin_ctzll(m); m &= m - 1; acc.insert((uint32_t)__shfl((int)key, l), acc_sc, acc_ss, lane); }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (acc.items != F.M) continue;                     // (the entries stay all ones)
        const uint32_t* const mg = g.merged_snp + F.out0;
        uint32_t* const out = g.set_order + F.out0;
        uint32_t k = 0;
        for (uint32_t i0 = 0; i0 < acc.buckets; i0 += 64) {
            const bool in = i0 + lane < acc.buckets;
            const uint32_t c = in ? acc.ctrl[i0 + lane] : 0xffu;
            const bool full = !(c & 0x80u);
            const uint64_t m = __ballot(full);
            const uint32_t j = k + mbcnt64(m);
            if (full && j < F.M) out[j] = asm_order_index(mg, F.M, acc.slot[i0 + lane]);
            k += (uint32_t)__popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the next fragment binds the tables anew
    }
}

// one thread per listed fragment: the same containers one insertion at a time, tables 0 / 1 the accumulator and its spare, 2 / 3 the growing map, 4 the part's set
__global__ __launch_bounds__(64) void assemble_order_general_kernel(AsmOrderArgs g) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_todo = g.todo[0] < g.n_frags ? g.todo[0] : g.n_frags;
    const uint64_t tb = g.ctrl_bytes + g.slot_bytes;
    if (tid >= g.n_threads || tid >= n_todo || (tid + 1) * AO_TABLES * tb > g.scratch_bytes) return;
    if (g.ctrl_bytes < fx_ctrl_bytes(g.cells_max + 1) || g.slot_bytes < fx_slot_bytes(g.cells_max + 1)) return;
    uint8_t* const mine = g.scratch + tid * AO_TABLES * tb;
    const auto ctrl_of = [&](uint32_t t) { return mine + t * tb; };
    const auto slot_of = [&](uint32_t t) { return (uint32_t*)(mine + t * tb + g.ctrl_bytes); };
    for (uint64_t ti = tid; ti < n_todo; ti += g.n_threads) {
        const uint64_t f = g.todo[1 + ti];
        AsmOrderFrag F;
        if (f >= g.n_frags || !asm_order_frag(g, f, F)) continue;
        uint64_t sum = 0;
        for (uint64_t p = F.p0; p < F.p1 && sum <= g.cells_max; ++p) { uint64_t b; sum += asm_order_part(g, p, b); }
        if (sum > g.cells_max || F.M > sum) continue;        // beyond the tables: the entries stay all ones
        FxTable acc;
        uint8_t* acc_sc = ctrl_of(1); uint32_t* acc_ss = slot_of(1);
        for (uint64_t p = F.p0; p < F.p1; ++p) {
            uint64_t b = 0;
            const uint32_t n = asm_order_part(g, p, b);                    // <= sum <= cells_max
            if (n == 0) continue;
            const uint32_t* ps = g.snp + b;
            const bool base = p == F.p0;
            FxTable seq;
            uint8_t* seq_sc = ctrl_of(3); uint32_t* seq_ss = slot_of(3);
            seq.bind(ctrl_of(2), slot_of(2), fx_buckets_for(1));
            for (uint32_t c = 0; c < n; ++c) seq.insert_new(ps[c], seq_sc, seq_ss);
            FxTable set;
            set.bind(ctrl_of(base ? 0 : 4), slot_of(base ? 0 : 4), fx_buckets_for(n));
            for (uint32_t i = 0; i < seq.buckets; ++i) if (!(seq.ctrl[i] & 0x80)) set.put(seq.slot[i]);
            if (base) { acc = set; continue; }
            if (acc.buckets == 0) acc.bind(ctrl_of(0), slot_of(0), fx_buckets_for(n));      // reserve(n) of the unallocated empty set
            else acc.reserve((n + 1) / 2, acc_sc, acc_ss);
            for (uint32_t i = 0; i < set.buckets; ++i) if (!(set.ctrl[i] & 0x80)) acc.insert(set.slot[i], acc_sc, acc_ss);
        }
        if (acc.items != F.M) continue;
        const uint32_t* const mg = g.merged_snp + F.out0;
        uint32_t* const out = g.set_order + F.out0;
        uint32_t k = 0;
        for (uint32_t i = 0; i < acc.buckets; ++i) if (!(acc.ctrl[i] & 0x80) && k < F.M) out[k++] = asm_order_index(mg, F.M, acc.slot[i]);
    }
}

}  // namespace fl
