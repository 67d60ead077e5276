// haploset_kernel.h — what follows S2's greedy re-insertion, on the device (floria_hip_reassign_batch_resident): the groups from `assign`,
// separate_broken_haplogroups (part_block_manip.rs:27-98) and sort_parts (:276-288), written into a floria_hip_haplosets handle.  The definition is the host code
// behind the kernel launch in floria_hip_reassign_batch; tests/haploset_model.py restates it and proves the scan form used here against the loops.
//
// INPUT GROUPS are numbered contig-major: k = grp_base[ci] + lg for group lg of contig ci.  A group's reads are the reads r of its contig with assign[r] == lg,
// ascending by id; every one of them sits in the group's input list, so a wavefront looks for them in the id window [rid_lo[k], rid_hi[k]) of that list only,
// a tile of 64 ids at a time: membership by ballot, ranks by prefix popcount — no atomics, nothing depends on the order in which anything lands.
//
// SPLITS as a scan.  The host walks a group's reads with `latest` = the maximum of `last` over the EARLIER reads and records a break (value `latest`) at a read with
// latest != 0 && first > latest && lo <= latest < hi.  The break values ascend strictly (after a break at r, latest >= last[r] >= first[r] > the break), and the
// second walk, which closes a part at the first read with last > end_spot and drops that read, closes it exactly at the read the break was recorded at: every
// earlier read has last <= that break value (it is their maximum) and the read itself has last >= first > it.  So: `latest` is an exclusive prefix maximum (carried
// across tiles in a wave-uniform register), a read with a break is dropped, every other read goes to part number (breaks at or before it), at the rank it has among
// the kept reads minus the rank the part starts at.  Part j of a group with breaks b_0 < .. < b_{n-1} spans (j ? b_{j-1} + 1 : lo, j < n ? b_j : hi).
//
// SLOTS, before the sort, per contig: its input groups in input order (a broken one stays, empty, with its range), then the parts of the broken groups in ascending
// group index.  With new_off the exclusive prefix sum over k of (breaks ? breaks + 1 : 0), contig ci's slots start at obase(ci) = grp_base[ci] + new_off[grp_base[ci]].
// SORT: rank of a slot = the number of slots of its contig with a smaller (lo, hi), or an equal one and a smaller slot index: std::stable_sort's order.  One thread per
// slot, the contig's keys streamed from L2 (a contig of BASELINE config 5 has a few thousand slots).
// Three walks (count, slots, fill) read `assign`, `first` and `last` of the window again instead of keeping per-read state: 12 B per read and walk.
// No LDS, no scratch; every launch is grid-stride over groups / slots ("chain_wgs" caps the grids).
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

struct HsArgs {
    const ContigDev* contigs;       // [n_contigs]
    const int32_t*   assign;        // the re-insertion's result: contig-local group id or -1, contig ci at assign_base[ci]
    const uint64_t*  assign_base;   // [n_contigs]
    const uint64_t*  grp_base;      // [n_contigs + 1] first input group of contig ci
    const uint32_t*  in_contig;     // [n_in]
    const uint32_t*  in_range;      // [2 * n_in] lo, hi
    const uint32_t*  rid_lo;        // [n_in] id window of the group's input list (rid_lo == rid_hi: no read)
    const uint32_t*  rid_hi;
    uint64_t*        new_off;       // [n_in + 1] COUNT: parts group k breaks into (0: not broken); then scanned in place
    uint64_t*        kept_off;      // [n_in + 1] COUNT: reads group k keeps; then scanned in place
    uint64_t*        counts;        // [2 * n_contigs] (groups, reads) of contig ci in the handle
    uint32_t*        slot_a;        // [n_out] rank among its input group's kept reads at which the slot starts
    uint32_t*        slot_b;        // [n_out] ... ends
    uint32_t*        slot_range;    // [2 * n_out]
    uint32_t*        slot_dst;      // [n_out] the slot's place in the handle
    uint32_t*        grp_contig;    // the handle's arrays
    uint64_t*        grp_off;       // [n_out + 1] RANK: sizes in final order; then scanned in place
    uint32_t*        grp_read;      // [n_reads_out]
    uint32_t*        range;         // [2 * n_out]
    uint64_t         n_out, n_reads_out;
    uint32_t         n_contigs, n_in;
    uint32_t         split;         // 0: "s2_assign_only" — no break is ever recorded and RANK keeps the slot order
};

struct HsWalk { uint32_t latest, kept, brks; };                      // wave-uniform: carried from tile to tile
struct HsLane { bool member, brk; uint32_t kept_before, brks_incl, latest; };

// one tile of 64 read ids of group lg: `in` = this lane's id lies in the window
__device__ __forceinline__ HsLane hs_tile(HsWalk& w, const int32_t* as, const ContigDev& cd, uint32_t r, bool in, uint32_t lg, uint32_t lo, uint32_t hi, bool split, uint32_t lane) {
    const bool member = in && G(as)[r] == (int32_t)lg;
    uint32_t f = 0, inc = 0;
    if (member) { f = G(cd.first)[r]; inc = G(cd.last)[r]; }
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t a = __shfl_up(inc, d, 64); if (lane >= d && a > inc) inc = a; }
    uint32_t ex = __shfl_up(inc, 1, 64);
    if (lane == 0 || ex < w.latest) ex = w.latest;
    const bool brk = split && member && ex != 0 && f > ex && ex >= lo && ex < hi;
    const uint64_t bm = __ballot(brk), km = __ballot(member) & ~bm;
    const HsLane o{member, brk, w.kept + mbcnt64(km), w.brks + mbcnt64(bm) + (brk ? 1u : 0u), ex};
    const uint32_t top = __shfl(inc, 63, 64);
    w.latest = top > w.latest ? top : w.latest; w.kept += (uint32_t)__popcll(km); w.brks += (uint32_t)__popcll(bm);
    return o;
}

__global__ __launch_bounds__(256) void hs_count_kernel(HsArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6); k < g.n_in; k += nw) {
        const uint32_t ci = g.in_contig[k], lg = k - (uint32_t)g.grp_base[ci], lo = g.in_range[2 * (uint64_t)k], hi = g.in_range[2 * (uint64_t)k + 1];
        const ContigDev cd = g.contigs[ci];
        const int32_t* as = g.assign + g.assign_base[ci];
        const uint32_t r1 = g.rid_hi[k] < cd.n_reads ? g.rid_hi[k] : cd.n_reads;
        HsWalk w{0, 0, 0};
        for (uint32_t r0 = g.rid_lo[k]; r0 < r1; r0 += 64) (void)hs_tile(w, as, cd, r0 + lane, r1 - r0 > lane, lg, lo, hi, g.split != 0, lane);
        if (lane == 0) { g.new_off[k] = w.brks ? w.brks + 1 : 0; g.kept_off[k] = w.kept; }
    }
}

// after the two scans: what the host sizes the handle by (and splits a download by)
__global__ __launch_bounds__(256) void hs_contig_counts_kernel(HsArgs g) {
    for (uint32_t ci = blockIdx.x * 256 + threadIdx.x; ci < g.n_contigs; ci += gridDim.x * 256) {
        const uint64_t a = g.grp_base[ci], b = g.grp_base[ci + 1];
        g.counts[2 * ci] = (b - a) + (g.new_off[b] - g.new_off[a]);
        g.counts[2 * ci + 1] = g.kept_off[b] - g.kept_off[a];
    }
}

// where the slots of group k lie: its own (s0), its parts' (pbase, nb of them)
struct HsSlots { uint64_t s0, pbase; uint32_t nb; };
__device__ __forceinline__ HsSlots hs_slots(const HsArgs& g, uint32_t k, uint32_t ci) {
    const uint64_t a = g.grp_base[ci], na = g.new_off[a], obase = a + na;
    return HsSlots{obase + (k - a), obase + (g.grp_base[ci + 1] - a) + (g.new_off[k] - na), (uint32_t)(g.new_off[k + 1] - g.new_off[k])};
}

__global__ __launch_bounds__(256) void hs_slots_kernel(HsArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6); k < g.n_in; k += nw) {
        const uint32_t ci = g.in_contig[k], lg = k - (uint32_t)g.grp_base[ci], lo = g.in_range[2 * (uint64_t)k], hi = g.in_range[2 * (uint64_t)k + 1];
        const ContigDev cd = g.contigs[ci];
        const int32_t* as = g.assign + g.assign_base[ci];
        const HsSlots S = hs_slots(g, k, ci);
        const uint32_t r1 = g.rid_hi[k] < cd.n_reads ? g.rid_hi[k] : cd.n_reads;
        HsWalk w{0, 0, 0};
        for (uint32_t r0 = g.rid_lo[k]; r0 < r1; r0 += 64) {
            const HsLane t = hs_tile(w, as, cd, r0 + lane, r1 - r0 > lane, lg, lo, hi, g.split != 0, lane);
            if (t.brk && t.brks_incl < S.nb && S.pbase + t.brks_incl < g.n_out) {      // break number brks_incl - 1 ends that part and starts the next
                const uint64_t p = S.pbase + t.brks_incl;
                g.slot_range[2 * p - 1] = t.latest; g.slot_range[2 * p] = t.latest + 1;
                g.slot_b[p - 1] = t.kept_before; g.slot_a[p] = t.kept_before;
            }
        }
        if (lane == 0 && S.s0 < g.n_out) {
            g.slot_range[2 * S.s0] = lo; g.slot_range[2 * S.s0 + 1] = hi;
            g.slot_a[S.s0] = 0; g.slot_b[S.s0] = S.nb ? 0 : w.kept;
            if (S.nb && S.pbase + S.nb <= g.n_out) {
                g.slot_range[2 * S.pbase] = lo; g.slot_a[S.pbase] = 0;
                g.slot_range[2 * (S.pbase + S.nb - 1) + 1] = hi; g.slot_b[S.pbase + S.nb - 1] = w.kept;
            }
        }
    }
}

__device__ __forceinline__ uint64_t hs_obase(const HsArgs& g, uint32_t c) { const uint64_t a = g.grp_base[c]; return a + g.new_off[a]; }

__global__ __launch_bounds__(256) void hs_rank_kernel(HsArgs g) {
    const uint2* key = (const uint2*)g.slot_range;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < g.n_out; s += (uint64_t)gridDim.x * 256) {
        uint32_t a = 0, z = g.n_contigs;                    // the slot's contig: the number of c in [1, n_contigs] with obase(c) <= s
        while (a < z) { const uint32_t mid = a + ((z - a) >> 1); if (hs_obase(g, mid + 1) <= s) a = mid + 1; else z = mid; }
        if (a >= g.n_contigs) continue;
        const uint64_t base = hs_obase(g, a), end = hs_obase(g, a + 1) < g.n_out ? hs_obase(g, a + 1) : g.n_out;
        const uint2 me = key[s];
        uint64_t rank = s - base;
        if (g.split) {
            rank = 0;
            for (uint64_t j = base; j < end; ++j) {
                const uint2 o = key[j];
                rank += (o.x < me.x || (o.x == me.x && (o.y < me.y || (o.y == me.y && j < s)))) ? 1 : 0;
            }
        }
        const uint64_t dst = base + rank;
        g.slot_dst[s] = (uint32_t)dst;
        g.range[2 * dst] = me.x; g.range[2 * dst + 1] = me.y;
        g.grp_contig[dst] = a;
        g.grp_off[dst] = g.slot_b[s] - g.slot_a[s];
    }
}

__global__ __launch_bounds__(256) void hs_fill_kernel(HsArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6); k < g.n_in; k += nw) {
        const uint32_t ci = g.in_contig[k], lg = k - (uint32_t)g.grp_base[ci], lo = g.in_range[2 * (uint64_t)k], hi = g.in_range[2 * (uint64_t)k + 1];
        const ContigDev cd = g.contigs[ci];
        const int32_t* as = g.assign + g.assign_base[ci];
        const HsSlots S = hs_slots(g, k, ci);
        const uint32_t r1 = g.rid_hi[k] < cd.n_reads ? g.rid_hi[k] : cd.n_reads;
        HsWalk w{0, 0, 0};
        for (uint32_t r0 = g.rid_lo[k]; r0 < r1; r0 += 64) {
            const HsLane t = hs_tile(w, as, cd, r0 + lane, r1 - r0 > lane, lg, lo, hi, g.split != 0, lane);
            const uint64_t s = S.nb ? S.pbase + t.brks_incl : S.s0;
            if (t.member && !t.brk && s < g.n_out) {
                const uint64_t at = g.grp_off[g.slot_dst[s]] + (t.kept_before - g.slot_a[s]);
                if (at < g.n_reads_out) g.grp_read[at] = r0 + lane;
            }
        }
    }
}

// floria_hip_hapq_batch_resident: the SNP span of every haploset's reads (min first, max last), one wavefront per group: lo[g], len[g] (0, 0 for a group without reads)
__global__ __launch_bounds__(256) void hs_span_kernel(const ContigDev* contigs, uint32_t n_contigs, const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read, uint32_t n_groups,
                                                      uint32_t* lo, uint32_t* len) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint32_t gi = blockIdx.x * 4 + (threadIdx.x >> 6); gi < n_groups; gi += nw) {
        const uint32_t ci = grp_contig[gi];
        uint32_t r0 = 0xffffffffu, r1 = 0;
        if (ci < n_contigs) {
            const ContigDev cd = contigs[ci];
            for (uint64_t i = grp_off[gi] + lane; i < grp_off[gi + 1]; i += 64) {
                const uint32_t r = grp_read[i];
                if (r < cd.n_reads) { const uint32_t f = G(cd.first)[r], l = G(cd.last)[r]; r0 = f < r0 ? f : r0; r1 = l > r1 ? l : r1; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t a = __shfl_xor(r0, o), b = __shfl_xor(r1, o); r0 = a < r0 ? a : r0; r1 = b > r1 ? b : r1; }
        if (lane == 0) { const bool any = !(r0 > r1); lo[gi] = any ? r0 : 0; len[gi] = any ? r1 - r0 + 1 : 0; }
    }
}

// ---- S2's input tables from a handle (floria_hip_reassign_haplosets_resident): what S2Plan::prologue builds on the host from group lists, built here from the
// handle's grp_contig / grp_off / grp_read.  Reads are numbered over all contigs: slot x = ro_base[ci] + r with ro_base[ci] = (reads of the contigs before ci) + ci, so
// every contig owns n_reads + 1 consecutive slots and the last one counts nothing: ONE exclusive scan over all slots then holds, for every contig, the n_reads + 1
// offsets of its read -> groups lists (absolute into r2g: the kernels' r2g_base is 0).
//   COUNT   a wavefront per group: ro[slot of the read] += 1 (integer atomicAdd: a count does not depend on the order);
//   FLAG    mf[x] = the read has a choice (count > 1); both arrays are then scanned (pileup_scan_*);
//   PLACE   a wavefront per group: the group's local id goes to its reads' lists at a cursor taken by atomicAdd, so a list holds the right SET in some order;
//   SORT    a thread per read: insertion sort of its list (a read has a handful of candidates) — ascending local group id, as the host's counting sort leaves it,
//           whatever order PLACE wrote in; the same thread writes the read into `multi` at the rank the scan of FLAG gave it: ascending visiting index;
//   RID     (hp_rid_kernel) a thread per group: the id window [first entry, last entry + 1) of its ascending list.
struct HpArgs {
    const ContigDev* contigs;
    const uint32_t*  grp_contig;    // the handle's arrays
    const uint64_t*  grp_off;
    const uint32_t*  grp_read;
    const uint64_t*  grp_base;      // [n_contigs] first group of contig ci
    const uint64_t*  ro_base;       // [n_contigs] first slot of contig ci
    uint64_t*        ro;            // [n_slots + 1] COUNT, then scanned in place
    uint64_t*        mf;            // [n_slots + 1] FLAG, then scanned in place
    uint32_t*        cursor;        // [n_slots - n_contigs] one per read, zeroed
    uint32_t*        r2g;           // [n_entries]
    uint32_t*        multi;         // [n_multi_cap]
    uint64_t*        multi_off;     // [n_contigs + 1]
    uint64_t         n_slots, n_entries, n_multi_cap;
    uint32_t         n_groups, n_contigs;
};

template <bool PLACE> __global__ __launch_bounds__(256) void hp_groups_kernel(HpArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint64_t k = blockIdx.x * 4 + (threadIdx.x >> 6); k < g.n_groups; k += nw) {
        const uint32_t ci = g.grp_contig[k];
        if (ci >= g.n_contigs) continue;
        const uint32_t N = g.contigs[ci].n_reads, lg = (uint32_t)(k - g.grp_base[ci]);
        const uint64_t base = g.ro_base[ci], i1 = g.grp_off[k + 1] < g.n_entries ? g.grp_off[k + 1] : g.n_entries;
        for (uint64_t i = g.grp_off[k] + lane; i < i1; i += 64) {
            const uint32_t r = g.grp_read[i];
            if (r >= N || base + r >= g.n_slots) continue;
            if (!PLACE) atomicAdd((unsigned long long*)&g.ro[base + r], 1ull);
            else {
                const uint64_t at = g.ro[base + r] + atomicAdd(&g.cursor[base - ci + r], 1u);      // (base - ci: the contig's first read among all reads)
                if (at < g.ro[base + r + 1] && at < g.n_entries) g.r2g[at] = lg;
            }
        }
    }
}

__global__ __launch_bounds__(256) void hp_flag_kernel(HpArgs g) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < g.n_slots; x += (uint64_t)gridDim.x * 256) g.mf[x] = g.ro[x] > 1 ? 1 : 0;
}

__global__ __launch_bounds__(256) void hp_sort_kernel(HpArgs g) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < g.n_slots; x += (uint64_t)gridDim.x * 256) {
        const uint64_t a = g.ro[x], b = g.ro[x + 1] < g.n_entries ? g.ro[x + 1] : g.n_entries;
        for (uint64_t i = a + 1; i < b; ++i) {
            const uint32_t v = g.r2g[i];
            uint64_t j = i;
            for (; j > a && g.r2g[j - 1] > v; --j) g.r2g[j] = g.r2g[j - 1];
            g.r2g[j] = v;
        }
        if (g.mf[x + 1] > g.mf[x] && g.mf[x] < g.n_multi_cap) {
            uint32_t lo = 0, hi = g.n_contigs;                  // the slot's contig: the last ci with ro_base[ci] <= x
            while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (g.ro_base[mid] <= x) lo = mid; else hi = mid; }
            g.multi[g.mf[x]] = (uint32_t)(x - g.ro_base[lo]);
        }
    }
}

__global__ __launch_bounds__(256) void hp_multi_off_kernel(HpArgs g) {
    for (uint64_t ci = (uint64_t)blockIdx.x * 256 + threadIdx.x; ci <= g.n_contigs; ci += (uint64_t)gridDim.x * 256) g.multi_off[ci] = ci < g.n_contigs ? g.mf[g.ro_base[ci]] : g.mf[g.n_slots];
}

__global__ __launch_bounds__(256) void hp_rid_kernel(const uint64_t* grp_off, const uint32_t* grp_read, uint32_t n_groups, uint64_t n_entries, uint32_t* rid_lo, uint32_t* rid_hi) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_groups; k += (uint64_t)gridDim.x * 256) {
        const uint64_t a = grp_off[k], b = grp_off[k + 1] < n_entries ? grp_off[k + 1] : n_entries;
        rid_lo[k] = b > a ? grp_read[a] : 0;
        rid_hi[k] = b > a ? grp_read[b - 1] + 1 : 0;
    }
}

}  // namespace fl
