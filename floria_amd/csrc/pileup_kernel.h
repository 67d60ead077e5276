// pileup_kernel.h — frag_from_record (file_reader.rs:661-736) for many alignment records at once: the CIGAR walk that turns a record into SNP calls
// (floria_hip_pileup_records).  For every M / = / X run [r, r + len) of a record every SNP of its contig inside the run yields one cell when the read
// base at q + (snp_pos - r) is one of the site's alleles; D / N consume the reference without a call, I / S the query only, H / P neither.
//
// One wavefront per record (grid-stride over the records), the CIGAR streamed 64 operations at a time:
//   * lane l reads operation k0 + l byte by byte (the words are not aligned in a BAM stream) and derives its (dq, dr);
//   * a wave inclusive scan (six __shfl_up steps) gives every operation its query / reference end inside the chunk; the running totals of the record
//     are wave-uniform; the chunk's prefix values go to the wave's slice of LDS (64 x {reference end, query end, the operation word});
//   * a wave-uniform cursor into the contig's ascending snp_pos starts at the first SNP >= pos (one 64-ary search per record: every probe round is a
//     coalesced load + ballot) and only moves forward.  The SNPs below the chunk's reference end are taken 64 per trip, one lane per SNP: a dense site
//     list under one long M takes several trips, a chunk without SNPs one load;
//   * a lane finds the operation that holds its SNP by a 6-step search over the chunk's 64 reference ends (the first end above the SNP: operations that do
//     not consume the reference repeat their predecessor's end and are never found), so there is no per-operation search of the SNP table and no loop whose
//     trip count differs between lanes;
//   * allele match, quality fetch and the stores are predicated; ballot + mbcnt give the write slots, so a record's cells ascend by SNP.
// The same walk runs twice, templated on the pass: COUNT leaves every record's number of cells in cell_off[], three small kernels turn the counts into exclusive
// offsets (tiles of 2048 records), FILL writes the exactly sized arrays.  No scratch, 20 B of LDS per lane.
// Every index is bounded by lengths the host validated before the launch (floria_hip_pileup_records): CIGAR bytes, sequence and quality bytes lie inside the
// blob, contig < n_contigs, snp_pos ascends strictly inside a contig, 1 <= n_alleles <= 4.
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

struct PileupArgs {
    const uint8_t*  blob;
    const int32_t*  pos;        // [n]
    const uint16_t* flags;      // [n]
    const uint32_t* contig;     // [n]
    const uint64_t* cigar_off;  // [n]
    const uint32_t* n_cigar;    // [n]
    const uint64_t* seq_off;    // [n]
    const uint32_t* l_seq;      // [n]
    const uint64_t* qual_off;   // [n]
    const uint64_t* snp_off;    // [n_contigs + 1]
    const int64_t*  snp_pos;    // [n_snps]
    const uint8_t*  alleles;    // [4 * n_snps] (the array starts on a 4-byte boundary)
    const uint8_t*  n_alleles;  // [n_snps]
    uint64_t* cell_off;         // [n + 1]  COUNT: cells per record (out); FILL: exclusive offsets (in)
    uint32_t* snp;              // FILL outputs, [cell_off[n]] each
    uint8_t*  allele;
    uint8_t*  qual;
    uint32_t* seq_pos;
    int64_t*  ref_end;          // [n]  written by the COUNT pass
    uint32_t  n_records;
};

constexpr uint32_t PILEUP_SCAN_TILE = 2048;      // records per tile of the offset scan (256 threads x 8)

// first index in [lo, hi) with snp_pos[index] >= key (hi if none); every argument and the result are wave-uniform
__device__ __forceinline__ uint64_t pileup_lower_bound(const int64_t* snp_pos, uint64_t lo, uint64_t hi, int64_t key, uint32_t lane) {
    // invariant: everything below lo is < key; hi is the end of the range or >= key
    while (hi - lo > 64) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t idx = lo + (uint64_t)lane * step;
        const bool lt = idx < hi && snp_pos[idx] < key;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(lt));       // the probes are ascending: the first cnt of them are < key
        if (cnt == 0) return lo;
        const uint64_t up = lo + (uint64_t)cnt * step;
        lo = lo + (uint64_t)(cnt - 1) * step + 1;
        hi = up < hi ? up : hi;
    }
    const uint64_t idx = lo + lane;
    const bool lt = idx < hi && snp_pos[idx] < key;
    return lo + (uint32_t)__popcll(__ballot(lt));
}

template <bool FILL>
__global__ __launch_bounds__(256) void pileup_walk_kernel(PileupArgs g) {
    __shared__ uint64_t s_rend[4][64], s_qend[4][64];
    __shared__ uint32_t s_word[4][64];
    const uint32_t lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    uint64_t* const rend = s_rend[wv];
    uint64_t* const qend = s_qend[wv];
    uint32_t* const word = s_word[wv];
    constexpr uint64_t NT16_LO = 0x565352474d43413dull, NT16_HI = 0x4e42444b48595754ull;      // "=ACMGRSV", "TWYHKDBN": the base of a 4-bit code
    const uint32_t n_waves = gridDim.x * 4;              // (the host keeps the grid far below 2^30 workgroups)
    for (uint32_t rec = blockIdx.x * 4 + wv; rec < g.n_records; rec += n_waves) {
        const int64_t pos = g.pos[rec];
        const uint32_t n_cig = g.n_cigar[rec], l_seq = g.l_seq[rec], c = g.contig[rec];
        const bool supp = (g.flags[rec] & 0x800u) != 0;
        const uint8_t* const cig = g.blob + g.cigar_off[rec];
        const uint8_t* const seq = g.blob + g.seq_off[rec];
        const uint8_t* const qual = g.blob + g.qual_off[rec];
        const uint64_t s1 = g.snp_off[c + 1];
        uint64_t cur = pileup_lower_bound(g.snp_pos, g.snp_off[c], s1, pos, lane);
        const uint32_t rank1 = 1u - (uint32_t)g.snp_off[c];      // SNP index -> rank in the contig + 1 (a contig has fewer than 2^32 SNPs: the low words suffice)
        uint64_t out = FILL ? g.cell_off[rec] : 0;       // next cell of the record (COUNT: how many so far)
        uint64_t q0 = 0;                                  // query / reference cursor in front of the chunk
        int64_t r0 = pos;
        uint32_t hard = 0;                                // leading hard clip of a supplementary alignment: added to seq_pos
        for (uint32_t k0 = 0; k0 < n_cig; k0 += 64) {
            const uint32_t k = k0 + lane;
            uint32_t w = 0;                               // (beyond the CIGAR: 0M, consumes nothing)
            if (k < n_cig) { const uint8_t* p = cig + 4 * (uint64_t)k; w = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
            const uint32_t op = w & 15u, len = w >> 4;
            if (k0 == 0) hard = rl32((supp && op == 5u) ? len : 0u, 0);
            // M I D N S H P = X: the query is consumed by M I S = X, the reference by M D N = X
            uint64_t iq = ((0x193u >> op) & 1u) ? len : 0u, ir = ((0x18du >> op) & 1u) ? len : 0u;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t a = __shfl_up((unsigned long long)iq, d, 64), b = __shfl_up((unsigned long long)ir, d, 64);
                if (lane >= d) { iq += a; ir += b; }
            }
            const uint64_t tq = rl64(iq, 63), tr = rl64(ir, 63);
            if (tr != 0 && cur < s1) {
                rend[lane] = ir; qend[lane] = iq; word[lane] = w;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (;;) {
                    const uint64_t idx = cur + lane;
                    uint64_t d = 0;                                                     // the SNP's offset from the chunk's first reference base
                    bool in = false;
                    if (idx < s1) { d = (uint64_t)g.snp_pos[idx] - (uint64_t)r0; in = d < tr; }      // (snp_pos >= r0: the cursor is past every SNP in front of the chunk)
                    const uint32_t n_in = (uint32_t)__popcll(__ballot(in));
                    if (n_in == 0) break;
                    bool emit = false;
                    uint32_t a_ix = 0;
                    uint64_t sp = 0;
                    if (in) {
                        uint32_t j = 0;                                               // the first operation whose reference end lies above the SNP
#pragma unroll
                        for (uint32_t s = 32; s > 0; s >>= 1) if (rend[j + s - 1] <= d) j += s;
                        const uint32_t wj = word[j], opj = wj & 15u, lenj = wj >> 4;
                        if (opj == 0u || opj == 7u || opj == 8u) {
                            sp = q0 + (qend[j] - lenj) + (d - (rend[j] - lenj));
                            if (sp < l_seq) {
                                const uint32_t byte = seq[sp >> 1], code = (sp & 1) ? (byte & 15u) : (byte >> 4);
                                const uint32_t base = (uint32_t)(((code & 8u) ? NT16_HI : NT16_LO) >> (8 * (code & 7u))) & 0xffu;
                                const uint32_t al = *(const uint32_t*)(g.alleles + 4 * idx), na = g.n_alleles[idx];
                                a_ix = na;
#pragma unroll
                                for (uint32_t t = 4; t-- > 0;) if (t < na && ((al >> (8 * t)) & 0xffu) == base) a_ix = t;      // the first matching allele wins
                                emit = a_ix < na;
                            }
                        }
                    }
                    const uint64_t em = __ballot(emit);
                    if (FILL && emit) {
                        const uint64_t slot = out + mbcnt64(em);
                        g.snp[slot] = (uint32_t)idx + rank1;
                        g.allele[slot] = (uint8_t)a_ix;
                        g.qual[slot] = qual[sp];
                        g.seq_pos[slot] = (uint32_t)(sp + hard);
                    }
                    out += (uint32_t)__popcll(em);
                    cur += n_in;
                    if (n_in < 64) break;
                }
                __builtin_amdgcn_wave_barrier();           // the next chunk overwrites the prefix values
            }
            q0 += tq; r0 += (int64_t)tr;
        }
        if (!FILL && lane == 0) { g.cell_off[rec] = out; g.ref_end[rec] = r0 != pos ? r0 : pos + 1; }      // (bam_endpos)
        if (n_waves >= g.n_records - rec) break;             // (rec + n_waves may not fit 32 bits)
    }
}

// ---- counts -> exclusive offsets: tile-local scan, scan of the tile sums, add ----------------------------------------------------------------
__global__ __launch_bounds__(256) void pileup_scan_tiles_kernel(uint64_t* v, uint64_t* tile_sum, uint32_t n) {
    __shared__ uint64_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * PILEUP_SCAN_TILE + (uint64_t)threadIdx.x * 8;
    uint64_t x[8], sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) { x[i] = base + i < n ? v[base + i] : 0; sum += x[i]; }
    uint64_t inc = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t a = __shfl_up((unsigned long long)inc, d, 64); if (lane >= d) inc += a; }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint64_t run = inc - sum;
    for (uint32_t k = 0; k < wv; ++k) run += s_wave[k];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) { if (base + i < n) v[base + i] = run; run += x[i]; }
    if (threadIdx.x == 255) tile_sum[blockIdx.x] = run;
}

// one workgroup: tile sums -> exclusive, the grand total behind the last record's offset
__global__ __launch_bounds__(256) void pileup_scan_sums_kernel(uint64_t* tile_sum, uint32_t n_tiles, uint64_t* total) {
    __shared__ uint64_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
        const uint32_t t = t0 + threadIdx.x;
        const uint64_t x = t < n_tiles ? tile_sum[t] : 0;
        uint64_t inc = x;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t a = __shfl_up((unsigned long long)inc, d, 64); if (lane >= d) inc += a; }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        uint64_t run = carry + inc - x;
        for (uint32_t k = 0; k < wv; ++k) run += s_wave[k];
        if (t < n_tiles) tile_sum[t] = run;
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void pileup_scan_add_kernel(uint64_t* v, const uint64_t* tile_sum, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] += tile_sum[i / PILEUP_SCAN_TILE];
}

}  // namespace fl
