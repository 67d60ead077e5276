// assemble_kernel.h — combine_frags (file_reader.rs:539-541, 636-639) on the cells of a resident pileup (floria_hip_assemble_contigs): a fragment is an ordered
// list of records ("parts") of floria_hip_pileup_records_resident; its cells are one cell per SNP that occurs in any part, ascending, allele and quality taken
// from the LAST part in list order that has the SNP (`seq_dict.extend` / `qual_dict.extend`: the later insertion overwrites), first / last the smallest and the
// largest merged SNP.  The merged cells go straight into the raw CSR regions of a batch arena laid out as an upload's (floria_hip.hip: plan_upload), where the
// existing flatten_kernel validates and flattens them as if they had come over the link.
//
// One wavefront per fragment (grid-stride over the fragments), no scratch, 8 B of LDS per lane:
//   * a fragment of ONE part is a straight copy of the record's cells;
//   * a fragment of several parts is merged by WINDOWS of 64 consecutive SNP indices [w, w + 64), lane l standing for SNP w + l.  The parts are visited in list
//     order (a wave-uniform loop: any number of parts).  For a part, one 64-ary search of its ascending SNP list (every probe round a coalesced load + ballot) gives
//     the first cell at or behind w; the part has at most 64 cells inside the window (its SNPs ascend strictly) and they are the next ones: lane l loads cell
//     i0 + l and, when its SNP s lies inside the window, writes its cell index into the wave's LDS slot s - w.  A later part overwrites an earlier one's slot:
//     that is the merge rule.  After the last part lane l reads slot l: ballot + mbcnt give the survivors' ranks, so the fragment's cells ascend;
//   * the next window starts at the smallest SNP at or behind w + 64 that any part has (a min over the cells the lanes loaded behind the window anyway), so a gap
//     between two mates or supplementary alignments costs one window, not one per 64 SNPs of the gap.
// The same merge runs twice, templated on the pass as pileup_walk_kernel is: COUNT leaves every fragment's number of merged cells in frag_cells[], the offset scan
// of pileup_kernel.h turns the counts into exclusive offsets over ALL fragments of the batch (the arena's cell regions are the contigs' back to back, so a global
// offset IS the cell's place), FILL writes snp / allele / qual there and the fragment's first, last and read_off entries.
// Every index is bounded by lengths the host validated before the launch: part_rec < n_records, offsets ascending, cell_off the device's own scan.
// With positions (the SP instance of FILL) the merged cell's SEQ_POS word goes next to its SNP: the sequence position of the cell
// that gave the SNP its call — `snp_pos_to_seq_pos.extend` follows the rule of `seq_dict.extend`, so it is the src[] slot the merge resolves anyway — and in
// bit 31 the mate flag of the part that cell belongs to, which rides in bit 63 of the slot (a cell index never reaches it).
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

struct AssembleArgs {
    // the resident pileup (pileup_walk_kernel<FILL>'s outputs)
    const uint64_t* cell_off;     // [n_records + 1]
    const uint32_t* snp;          // [cell_off[n_records]]
    const uint8_t*  allele;
    const uint8_t*  qual;
    // the fragment plan
    const uint64_t* part_off;     // [n_frags + 1] into part_rec
    const uint32_t* part_rec;     // record indices, merge order
    const uint32_t* frag_ctg;     // [n_frags] contig of the fragment
    const uint64_t* frag_off;     // [n_contigs + 1] fragments of contig c
    uint64_t* frag_cells;         // [n_frags + 1]  COUNT: merged cells per fragment (out); FILL: exclusive offsets over all fragments (in)
    // FILL outputs: the raw regions of the batch arena
    uint32_t* read_off;           // contig c's array [n_reads + 1] starts at entry frag_off[c] + c
    uint32_t* first;              // [n_frags]
    uint32_t* last;               // [n_frags]
    uint32_t* out_snp;            // [frag_cells[n_frags]]
    uint8_t*  out_allele;
    uint8_t*  out_qual;
    uint64_t  n_frags;
    // floria_hip_assemble_contigs_opt with KEEP_SEQ_POS (FILL only; all four null / unused otherwise): the word `mate << 31 | seq_pos` of every merged cell
    const uint32_t* seq_pos;      // [cell_off[n_records]] pileup_walk_kernel<FILL>'s seq_pos, next to snp
    const uint8_t*  part_mate;    // [part_off[n_frags]] 0 / 1 per part, null = all 0
    uint32_t* out_sp;             // [frag_cells[n_frags]] the arena's seq_pos region (the SP instance only)
    uint32_t* sp_overflow;        // one word, set to 1 when a walked seq_pos >= 2^31 was met (it cannot be encoded: the host refuses the call)
};

constexpr uint64_t ASM_NONE = ~0ull;

__device__ __forceinline__ uint64_t asm_wave_min(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32) | __shfl_xor((uint32_t)v, o);
        v = w < v ? w : v;
    }
    return v;
}

// first index in [lo, hi) with snp[index] >= key (hi if none); every argument and the result are wave-uniform (pileup_lower_bound for a cell list)
__device__ __forceinline__ uint64_t asm_lower_bound(const uint32_t* snp, uint64_t lo, uint64_t hi, uint64_t key, uint32_t lane) {
    while (hi - lo > 64) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t idx = lo + (uint64_t)lane * step;
        const bool lt = idx < hi && (uint64_t)snp[idx] < key;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(lt));       // the probes ascend: the first cnt of them are < key
        if (cnt == 0) return lo;
        const uint64_t up = lo + (uint64_t)cnt * step;
        lo = lo + (uint64_t)(cnt - 1) * step + 1;
        hi = up < hi ? up : hi;
    }
    const uint64_t idx = lo + lane;
    const bool lt = idx < hi && (uint64_t)snp[idx] < key;
    return lo + (uint32_t)__popcll(__ballot(lt));
}

// SP: the FILL instance that also writes the SEQ_POS words.  A template parameter, not a test of out_sp at run time: with the run-time branch the plain FILL pass
// (one-part fragments, the straight copy) measured 0.10 ms slower on the 200-contig long-read set than the kernel without the feature (profiles/read_spans.md), so
// the plain call launches an instance whose code has no trace of it; part_mate stays a nullable pointer behind a wave-uniform branch of the SP instance.
template <bool FILL, bool SP = false>
__global__ __launch_bounds__(256) void assemble_kernel(AssembleArgs g) {
    static_assert(FILL || !SP, "positions are written by the FILL pass");
    __shared__ uint64_t s_src[4][64];
    const uint32_t lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    uint64_t* const src = s_src[wv];                       // slot l: 1 + the cell that gives SNP w + l its call, 0 = no part has the SNP
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t f = (uint64_t)blockIdx.x * 4 + wv; f < g.n_frags; f += n_waves) {
        const uint64_t p0 = g.part_off[f], p1 = g.part_off[f + 1];
        const uint64_t out0 = FILL ? g.frag_cells[f] : 0;
        uint64_t out = out0;                               // next cell of the fragment (COUNT: how many so far)
        uint32_t lo_snp = 0, hi_snp = 0;
        if (p1 - p0 == 1) {                                // one part: the record's cells as they are
            const uint32_t rec = g.part_rec[p0];
            const uint64_t b = g.cell_off[rec], e = g.cell_off[rec + 1];
            if (FILL) {
                for (uint64_t c = b + lane; c < e; c += 64) {
                    const uint64_t slot = out0 + (c - b);
                    g.out_snp[slot] = g.snp[c]; g.out_allele[slot] = g.allele[c]; g.out_qual[slot] = g.qual[c];
                }
                if (SP) {
                    const uint32_t mate = g.part_mate ? (uint32_t)(g.part_mate[p0] & 1u) << 31 : 0u;
                    for (uint64_t c = b + lane; c < e; c += 64) {
                        const uint32_t sp = g.seq_pos[c];
                        if (sp >> 31) atomicOr(g.sp_overflow, 1u);
                        g.out_sp[out0 + (c - b)] = (sp & 0x7fffffffu) | mate;
                    }
                }
                if (e > b) { lo_snp = g.snp[b]; hi_snp = g.snp[e - 1]; }
            }
            out += e - b;
        } else {
            // the first window starts at the smallest SNP of any part (lanes over the parts, 64 at a time)
            uint64_t nx = ASM_NONE;
            for (uint64_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t rec = g.part_rec[p];
                const uint64_t b = g.cell_off[rec];
                if (g.cell_off[rec + 1] > b) { const uint64_t s = g.snp[b]; nx = s < nx ? s : nx; }
            }
            nx = asm_wave_min(nx);
            bool first_window = true;
            while (nx != ASM_NONE) {
                const uint64_t w = nx;
                src[lane] = 0;
                __builtin_amdgcn_wave_barrier();
                uint64_t cand = ASM_NONE;                  // the smallest SNP at or behind w + 64 this lane has seen
                for (uint64_t p = p0; p < p1; ++p) {
                    const uint32_t rec = g.part_rec[p];
                    const uint64_t b = g.cell_off[rec], e = g.cell_off[rec + 1];
                    if (e == b) continue;
                    const uint64_t mbit = SP && g.part_mate ? (uint64_t)(g.part_mate[p] & 1u) << 63 : 0ull;      // (wave-uniform)
                    const uint64_t i0 = asm_lower_bound(g.snp, b, e, w, lane);
                    const uint64_t idx = i0 + lane;
                    const uint64_t s = idx < e ? (uint64_t)g.snp[idx] : ASM_NONE;
                    const bool in = s != ASM_NONE && s - w < 64;      // (s >= w: idx is at or behind the lower bound)
                    if (in) src[s - w] = (idx + 1) | mbit; // LDS writes of one wave land in program order: the later part wins
                    else if (s < cand) cand = s;
                    if (__popcll(__ballot(in)) == 64 && i0 + 64 < e) {      // the window is full of this part: its next cell lies behind the 64 loaded ones
                        const uint64_t s2 = g.snp[i0 + 64];
                        cand = s2 < cand ? s2 : cand;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint64_t sv = src[lane], sc = SP ? sv & ~(1ull << 63) : sv;
                const bool have = sc != 0;
                const uint64_t m = __ballot(have);         // (bit 0 is set: w is a SNP some part has)
                if (FILL) {
                    if (have) {
                        const uint64_t slot = out + mbcnt64(m);
                        g.out_snp[slot] = (uint32_t)(w + lane); g.out_allele[slot] = g.allele[sc - 1]; g.out_qual[slot] = g.qual[sc - 1];
                        if (SP) {
                            const uint32_t sp = g.seq_pos[sc - 1];
                            if (sp >> 31) atomicOr(g.sp_overflow, 1u);
                            g.out_sp[slot] = (sp & 0x7fffffffu) | ((uint32_t)(sv >> 63) << 31);
                        }
                    }
                    if (first_window) lo_snp = (uint32_t)w;
                    hi_snp = (uint32_t)(w + 63 - (uint32_t)__clzll((long long)m));
                }
                first_window = false;
                out += (uint32_t)__popcll(m);
                __builtin_amdgcn_wave_barrier();           // the next window clears the slots
                nx = asm_wave_min(cand);
            }
        }
        if (lane == 0) {
            if (!FILL) g.frag_cells[f] = out;
            else {
                const uint32_t c = g.frag_ctg[f];
                const uint64_t f0 = g.frag_off[c], base = g.frag_cells[f0];      // the contig's first fragment and first cell
                g.first[f] = lo_snp; g.last[f] = hi_snp;
                g.read_off[f + c] = (uint32_t)(out0 - base);
                if (f + 1 == g.frag_off[c + 1]) g.read_off[f + 1 + c] = (uint32_t)(out - base);
            }
        }
    }
}

// per-contig cell totals for the arena plan: tot[c] = the exclusive offset of contig c's first fragment (c = n_contigs: all cells)
__global__ __launch_bounds__(256) void assemble_totals_kernel(const uint64_t* frag_cells, const uint64_t* frag_off, uint64_t* tot, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) tot[i] = frag_cells[frag_off[i]];
}

// floria_hip_pileup_records_resident: the SNP of every record's first and last cell (0 / 0 for a record without cells), from the FILL pass's output
__global__ __launch_bounds__(256) void record_span_kernel(const uint64_t* cell_off, const uint32_t* snp, uint32_t* first_snp, uint32_t* last_snp, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = cell_off[i], e = cell_off[i + 1];
    first_snp[i] = e > b ? snp[b] : 0u;
    last_snp[i] = e > b ? snp[e - 1] : 0u;
}

}  // namespace fl
