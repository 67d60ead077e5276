// mono_kernel.h — remove_monomorphic_allele (utils_frags.rs:713-772, --ignore-monomorphic) on resident contigs (floria_hip_drop_monomorphic): the phred weights of
// every (SNP, allele) are summed over all reads, a SNP with one allele only or with `heaviest * error > second` is removed from every read, reads left without
// cells are dropped and the survivors re-sorted by Frag::cmp.  The inputs are resident contigs (any arenas), the outputs one new batch arena laid out as an
// upload's (floria_hip.hip: plan_upload) and written in the RESIDENT form directly: the raw allele / quality bytes an upload flattens no longer exist, so FILL
// below restates flatten_kernel's per-read outputs (cell_aw as it is, the tw sums, the 32-B meta record, the per-contig status words).
//
//   mono_count_kernel          16 lanes per read (the frame of flatten_kernel).  A cell's weight is the Q24 field of cell_aw: wsum[4 * SNP + allele] += w, a
//                              returnless 64-bit integer atomic (integer adds are order-free: the table is bit-reproducible).  A q = 0 cell weighs 0 but makes its
//                              allele a key of the reference's map all the same: it sets the allele's bit in zero_key[SNP] instead (a weight > 0 implies presence,
//                              so one atomic per cell either way).
//   mono_decide_kernel         one thread per SNP: present alleles = weight > 0 or zero-key bit; none -> kept (the SNP is not in the map), one -> removed, else
//                              removed iff (double)S0 * 2^-24 * error > (double)S1 * 2^-24 for the two largest sums (strict; exact below 2^53).
//   mono_filter_kernel<false>  COUNT, 16 lanes per INPUT read: surviving cells, first and last surviving SNP: three words per read, all the host sees of a read.
//                              The host drops the empty reads, sorts the rest per contig (first ascending, last descending, old index ascending), takes the prefix
//                              sums and sends read_off and old_read back.
//   mono_filter_kernel<true>   FILL, one wavefront per OUTPUT read: ballot + mbcnt compaction of the surviving cells into the read's place, first / last, the tw
//                              sums, the meta record, the contig's status words.  Where the input contig carries positions the surviving cells' SEQ_POS words move
//                              with them (the reference removes the key from snp_pos_to_seq_pos with the cell, utils_frags.rs:749).
//   mono_order_kernel          only when set orders are asked for, one wavefront per output read, after FILL (it reads the SNP list FILL wrote): the input read's
//                              cells in set order (cell_orders' output) with the removed ones deleted, each renumbered to its index in the cut-down read.
// Every index is bounded by lengths the host validated before the launch (cells per contig, SNPs per contig: no `last` exceeds its contig's SNP count) and, where a
// value comes out of device memory (an SNP index, a read's cell range), compared against that length once more before it addresses anything.
#pragma once
#include "common.h"
#include "wave_util.h"
#include "upload_kernel.h"

namespace fl {

struct MonoContig {                // one input contig and its place in the tables
    const uint32_t* read_off;      // [n_reads+1]
    const uint32_t* snp;           // [n_cells]
    const uint32_t* cell_aw;       // [n_cells]
    uint64_t snp_base;             // snp_off[c]: the contig's first entry of wsum / 4, zero_key and removed
    uint64_t ord_base;             // cells of the contigs before it: where its part of the cell orders starts
    uint32_t n_reads, n_cells, n_snps, pad;
    const uint32_t* seq_pos;       // [n_cells] the SEQ_POS words of a contig that carries positions, else null
};

struct MonoArgs {
    const MonoContig* contigs;
    const uint64_t* read_prefix;   // [n_contigs+1] input reads before contig c
    const uint64_t* snp_off;       // [n_contigs+1]
    unsigned long long* wsum;      // [4 * n_snps_total] Q24 weight sums
    uint32_t* zero_key;            // [n_snps_total] bit a: some cell of weight 0 calls allele a
    uint8_t*  removed;             // [n_snps_total]
    unsigned long long* n_removed; // [n_contigs] removed SNPs
    uint32_t* keep3;               // [3 * n_reads_in] COUNT: surviving cells, first, last of every input read
    double    error;
    uint64_t  n_reads_in, n_snps_total;
    uint32_t  n_contigs, pad;
    // FILL / ORDER: the output batch
    const UploadContig* out;       // the regions of the new arena per contig (allele / qual unused; read_off filled by the host's copy)
    const uint64_t* out_prefix;    // [n_contigs+1] output reads before contig c
    const uint32_t* old_read;      // [n_reads_out] input read (index inside its contig) of every output read
    UploadStatus* status;          // [n_contigs]
    const uint64_t *Rq1, *Rq2;
    uint32_t* const* out_set_order;// [n_contigs] (ORDER) the contig's set_order region
    const uint2* ord;              // (ORDER) the input contigs' cells in set order
    uint64_t  n_reads_out;
    uint32_t* const* out_seq_pos;  // [n_contigs] (FILL) the contig's seq_pos region, null where its input carries none; the table itself null when no input does
};

// is SNP s (1-based, as read from a cell) of contig cd removed?  An index outside the contig's table counts as removed: it addresses nothing.
__device__ __forceinline__ bool mono_gone(const MonoArgs& g, const MonoContig& cd, uint32_t s) {
    const uint32_t i = s - 1u;
    return i >= cd.n_snps || G(g.removed)[cd.snp_base + i] != 0;
}

__global__ __launch_bounds__(64) void mono_count_kernel(MonoArgs g) {
    const uint32_t lane = threadIdx.x, sub = lane & 15, grp = lane >> 4;
    const uint64_t lr0 = (uint64_t)blockIdx.x * UP_READS_PER_WG;
    uint32_t ci = wave_find_contig(g.read_prefix, g.n_contigs, lr0, lane);
    for (int it = 0; it < UP_READS_PER_WG / 4; ++it) {
        const uint64_t lr = lr0 + (uint64_t)it * 4 + grp;
        if (lr >= g.n_reads_in) continue;
        while (g.read_prefix[ci + 1] <= lr) ++ci;
        const MonoContig cd = g.contigs[ci];
        const uint32_t r = (uint32_t)(lr - g.read_prefix[ci]);
        const uint32_t b = G(cd.read_off)[r];
        uint32_t e = G(cd.read_off)[r + 1];
        e = e > cd.n_cells ? cd.n_cells : e;
        for (uint32_t c = b + sub; c < e; c += 16) {
            const uint32_t i = G(cd.snp)[c] - 1u, aw = G(cd.cell_aw)[c];
            if (i >= cd.n_snps) continue;
            const uint32_t a = (aw >> 28) & 3u, w = aw & 0x0fffffffu;
            const uint64_t k = cd.snp_base + i;
            if (w) (void)__hip_atomic_fetch_add(&g.wsum[4 * k + a], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_fetch_or(&g.zero_key[k], 1u << a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(256) void mono_decide_kernel(MonoArgs g) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= g.n_snps_total) return;
    const ulonglong2 s01 = *(const ulonglong2*)(g.wsum + 4 * k), s23 = *(const ulonglong2*)(g.wsum + 4 * k + 2);
    const unsigned long long s[4] = {s01.x, s01.y, s23.x, s23.y};
    const uint32_t zk = g.zero_key[k];
    uint32_t n = 0;
    unsigned long long v0 = 0, v1 = 0;                    // the two largest sums among the present alleles, v0 >= v1
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!(s[a] != 0 || ((zk >> a) & 1u))) continue;
        ++n;
        if (s[a] > v0) { v1 = v0; v0 = s[a]; } else if (s[a] > v1) v1 = s[a];
    }
    bool gone = n == 1;
    if (n >= 2) gone = ((double)v0 * 0x1p-24) * g.error > (double)v1 * 0x1p-24;
    g.removed[k] = gone ? 1 : 0;
    if (gone) {
        uint32_t lo = 0, hi = g.n_contigs;                  // contig of table entry k: the last c with snp_off[c] <= k
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (g.snp_off[mid] <= k) lo = mid; else hi = mid; }
        (void)__hip_atomic_fetch_add(&g.n_removed[lo], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool FILL> __global__ void mono_filter_kernel(MonoArgs g);

// COUNT: per input read
template <> __global__ __launch_bounds__(64) void mono_filter_kernel<false>(MonoArgs g) {
    const uint32_t lane = threadIdx.x, sub = lane & 15, grp = lane >> 4;
    const uint64_t lr0 = (uint64_t)blockIdx.x * UP_READS_PER_WG;
    uint32_t ci = wave_find_contig(g.read_prefix, g.n_contigs, lr0, lane);
    for (int it = 0; it < UP_READS_PER_WG / 4; ++it) {
        const uint64_t lr = lr0 + (uint64_t)it * 4 + grp;
        const bool live = lr < g.n_reads_in;
        uint32_t cnt = 0, lo = 0xffffffffu, hi = 0;
        if (live) {
            while (g.read_prefix[ci + 1] <= lr) ++ci;
            const MonoContig cd = g.contigs[ci];
            const uint32_t r = (uint32_t)(lr - g.read_prefix[ci]);
            const uint32_t b = G(cd.read_off)[r];
            uint32_t e = G(cd.read_off)[r + 1];
            e = e > cd.n_cells ? cd.n_cells : e;
            for (uint32_t c = b + sub; c < e; c += 16) {
                const uint32_t s = G(cd.snp)[c];
                if (mono_gone(g, cd, s)) continue;
                ++cnt; lo = s < lo ? s : lo; hi = s > hi ? s : hi;
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const uint32_t oc = __shfl_xor(cnt, o), ol = __shfl_xor(lo, o), oh = __shfl_xor(hi, o);
            cnt += oc; lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
        }
        if (live && sub == 0) { uint32_t* k3 = g.keep3 + 3 * lr; k3[0] = cnt; k3[1] = cnt ? lo : 0u; k3[2] = hi; }
    }
}

// The contig of output read gr (wave-uniform): the last c with out_prefix[c] <= gr.  A wavefront's reads ascend along its grid-stride loop, so it searches once
// (wave_find_contig: all lanes sample the prefix array at once) and then only steps forward.
__device__ __forceinline__ uint32_t mono_out_contig(const MonoArgs& g, uint64_t gr, uint32_t ci) {
    while (g.out_prefix[ci + 1] <= gr) ++ci;                 // (ends: out_prefix[n_contigs] = n_reads_out > gr)
    return ci;
}

// FILL: per output read
template <> __global__ __launch_bounds__(256) void mono_filter_kernel<true>(MonoArgs g) {
    const uint32_t lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint64_t gr0 = (uint64_t)blockIdx.x * 4 + wv;
    if (gr0 >= g.n_reads_out) return;
    uint32_t ci = uni(wave_find_contig(g.out_prefix, g.n_contigs, gr0, lane));
    for (uint64_t gr = gr0; gr < g.n_reads_out; gr += n_waves) {
        ci = mono_out_contig(g, gr, ci);
        const MonoContig cd = g.contigs[ci];
        const UploadContig od = g.out[ci];
        const uint32_t r = (uint32_t)(gr - g.out_prefix[ci]), ro = g.old_read[gr];
        if (ro >= cd.n_reads) continue;
        const uint32_t b = G(cd.read_off)[ro];
        uint32_t e = G(cd.read_off)[ro + 1];
        e = e > cd.n_cells ? cd.n_cells : e;
        const uint32_t ob = G(od.read_off)[r];
        uint32_t* const osp = g.out_seq_pos && cd.seq_pos ? g.out_seq_pos[ci] : nullptr;      // (wave-uniform)
        uint32_t n = 0, F = 0, L = 0, ma = 0, q0 = 0;          // n, F, L wave-uniform
        uint64_t t1 = 0, t2 = 0;
        for (uint32_t c0 = b; c0 < e; c0 += 64) {
            const uint32_t c = c0 + lane;
            const bool v = c < e;
            const uint32_t s = v ? G(cd.snp)[c] : 0u, aw = v ? G(cd.cell_aw)[c] : 0u;
            const bool keep = v && !mono_gone(g, cd, s);
            const uint64_t m = __ballot(keep);
            if (m == 0) continue;
            const uint64_t slot = (uint64_t)ob + n + mbcnt64(m);
            if (keep && slot < od.n_cells) {
                const uint32_t a = (aw >> 28) & 3u, w = aw & 0x0fffffffu;
                const uint32_t idx = hash_idx(s, a);
                ((uint32_t*)od.snp)[slot] = s; od.cell_aw[slot] = aw;
                if (osp) osp[slot] = G(cd.seq_pos)[c];
                t1 += g.Rq1[idx] * (uint64_t)w; t2 += g.Rq2[idx] * (uint64_t)w;
                ma = a > ma ? a : ma; q0 |= w == 0 ? 1u : 0u;
            }
            if (n == 0) F = rl32(s, (uint32_t)__ffsll((long long)m) - 1u);
            L = rl32(s, 63u - (uint32_t)__clzll((long long)m));
            n += (uint32_t)__popcll(m);
        }
        t1 = wave_sum_u64(t1); t2 = wave_sum_u64(t2);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t om = __shfl_xor(ma, o), oq = __shfl_xor(q0, o); ma = om > ma ? om : ma; q0 |= oq; }
        if (lane == 0) {
            ((uint32_t*)od.first)[r] = F; ((uint32_t*)od.last)[r] = L;
            od.tw[2 * (uint64_t)r] = t1; od.tw[2 * (uint64_t)r + 1] = t2;
            uint32_t* mr = od.meta + 8 * (uint64_t)r;
            *(uint4*)mr = make_uint4(ob, n, F, L);
            *(uint4*)(mr + 4) = make_uint4((uint32_t)t1, (uint32_t)(t1 >> 32), (uint32_t)t2, (uint32_t)(t2 >> 32));
            UploadStatus* st = g.status + ci;
            atomicMax(&st->max_len, n);
            if (ma) atomicMax(&st->max_allele, ma);
            if (q0) atomicOr(&st->has_q0, 1u);
        }
    }
}

// ORDER: the set order of every output read = the input read's with the removed cells deleted, renumbered
__global__ __launch_bounds__(256) void mono_order_kernel(MonoArgs g) {
    const uint32_t lane = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint64_t gr0 = (uint64_t)blockIdx.x * 4 + wv;
    if (gr0 >= g.n_reads_out) return;
    uint32_t ci = uni(wave_find_contig(g.out_prefix, g.n_contigs, gr0, lane));
    for (uint64_t gr = gr0; gr < g.n_reads_out; gr += n_waves) {
        ci = mono_out_contig(g, gr, ci);
        const MonoContig cd = g.contigs[ci];
        const UploadContig od = g.out[ci];
        uint32_t* const so = g.out_set_order[ci];
        const uint32_t r = (uint32_t)(gr - g.out_prefix[ci]), ro = g.old_read[gr];
        if (ro >= cd.n_reads || !so) continue;
        const uint32_t b = G(cd.read_off)[ro];
        uint32_t e = G(cd.read_off)[ro + 1];
        e = e > cd.n_cells ? cd.n_cells : e;
        const uint32_t ob = G(od.read_off)[r];
        uint32_t oe = G(od.read_off)[r + 1];
        oe = oe > od.n_cells ? od.n_cells : oe;
        const uint32_t n = oe > ob ? oe - ob : 0u;
        const uint32_t* const mine = od.snp + ob;           // the read's surviving SNPs, ascending (FILL)
        const uint2* const ord = g.ord + cd.ord_base + b;
        uint32_t k = 0;
        for (uint32_t x0 = 0; x0 < e - b && b < e; x0 += 64) {
            const uint32_t x = x0 + lane;
            const bool v = x < e - b;
            const uint32_t s = v ? ord[x].x : 0u;
            const bool keep = v && !mono_gone(g, cd, s);
            uint32_t lo = 0, hi = n;                           // index of s among the survivors
            if (keep) while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (G(mine)[mid] < s) lo = mid + 1; else hi = mid; }
            const uint64_t m = __ballot(keep);
            const uint32_t at = k + mbcnt64(m);
            if (keep && at < n) so[ob + at] = lo;
            k += (uint32_t)__popcll(m);
        }
    }
}

}  // namespace fl
