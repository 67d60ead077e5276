// path_kernel.h — the union at the end of get_disjoint_paths_rewrite (graph_processing.rs; host/stitch.cpp:283-295) on the device (floria_hip_join_paths): a path
// is a list of hap-graph nodes (block, partition) of the S1 batch that is still resident; its haploset is every read some node (b, k) of it lists with part == k,
// ascending and once each.  The block lists (BlockSet::blk_read, ascending ids) and the partition bytes are the ones floria_hip_hap_graph reads.
//
// WINDOW  per path, one wavefront: [lo, hi) = from the smallest first entry to the largest last entry + 1 of its nodes' block lists — every read of the path lies in
//         it; the path owns ceil((hi - lo) / 64) words of ONE bitmap (memory linear in the sum of the windows), word_off = their exclusive prefix sum.
// MARK    per (path, node), one wavefront, 64 list entries a trip: an entry with part == k sets bit (id - lo) of its path's words by atomicOr.  A read two nodes
//         of a path share sets the same bit twice: the union needs no other dedupe, and an OR does not depend on the order in which anything lands.
// COUNT   per path, one wavefront: popcount over its words = the group's size; scanned (pileup_scan_*) into the handle's grp_off.
// FILL    per path, one wavefront, 64 words a trip: a lane ranks its word by the prefix popcount of the lanes below it plus the carry of the earlier trips and writes
//         the ids of its set bits, ascending, from that rank on.
// No LDS, no scratch, no float; integer atomicOr is the only atomic.  Every launch is grid-stride ("chain_wgs" caps the grids); every index that comes from
// memory is bounded by the lengths the host passed before it is used as an address.
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

struct PathArgs {
    BlockSet        bs;             // the resident S1 batch
    const uint8_t*  part;           // [blk_read_off[n_blocks]] partition of every list entry
    const uint64_t* node_off;       // [n_paths + 1]
    const uint32_t* node_block;     // [n_nodes]
    const uint8_t*  node_part;      // [n_nodes]
    const uint32_t* node_path;      // [n_nodes] the path a node belongs to
    const uint64_t* path_base;      // [n_contigs + 1] first path of contig ci
    uint32_t*       win_lo;         // [n_paths] WINDOW
    uint64_t*       word_off;       // [n_paths + 1] WINDOW: words of the path; then scanned in place
    uint64_t*       bitmap;         // [n_words], zeroed
    uint64_t*       grp_off;        // [n_paths + 1] COUNT: reads of the path; then scanned in place
    uint64_t*       counts;         // [2 * n_contigs] (groups, reads) of contig ci
    uint32_t*       grp_read;       // [n_reads_out]
    uint64_t        n_words, n_reads_out, n_nodes;
    uint32_t        n_paths, n_contigs;
};

__global__ __launch_bounds__(256) void path_window_kernel(PathArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint64_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < g.n_paths; p += nw) {
        uint32_t lo = 0xffffffffu, hi = 0;
        const uint64_t n1 = g.node_off[p + 1] < g.n_nodes ? g.node_off[p + 1] : g.n_nodes;
        for (uint64_t n = g.node_off[p] + lane; n < n1; n += 64) {
            const uint32_t b = g.node_block[n];
            if (b >= g.bs.n_blocks) continue;
            const uint64_t a = g.bs.blk_read_off[b], z = g.bs.blk_read_off[b + 1];
            if (z > a) { const uint32_t f = g.bs.blk_read[a], l = g.bs.blk_read[z - 1]; lo = f < lo ? f : lo; hi = l >= hi ? l + 1 : hi; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t a = __shfl_xor(lo, o), b = __shfl_xor(hi, o); lo = a < lo ? a : lo; hi = b > hi ? b : hi; }
        if (lane == 0) { const bool any = hi > lo; g.win_lo[p] = any ? lo : 0; g.word_off[p] = any ? ((uint64_t)(hi - lo) + 63) / 64 : 0; }
    }
}

__global__ __launch_bounds__(256) void path_mark_kernel(PathArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint64_t n = blockIdx.x * 4 + (threadIdx.x >> 6); n < g.n_nodes; n += nw) {
        const uint32_t p = g.node_path[n], b = g.node_block[n], k = g.node_part[n];
        if (p >= g.n_paths || b >= g.bs.n_blocks) continue;
        const uint32_t lo = g.win_lo[p];
        const uint64_t w0 = g.word_off[p], nwords = g.word_off[p + 1] - w0;
        const uint64_t z = g.bs.blk_read_off[b + 1];
        for (uint64_t i = g.bs.blk_read_off[b] + lane; i < z; i += 64) {
            if (g.part[i] != k) continue;
            const uint32_t r = g.bs.blk_read[i];
            const uint64_t w = ((uint64_t)r - lo) >> 6;
            if (r >= lo && w < nwords && w0 + w < g.n_words) atomicOr((unsigned long long*)&g.bitmap[w0 + w], 1ull << ((r - lo) & 63));
        }
    }
}

__global__ __launch_bounds__(256) void path_count_kernel(PathArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint64_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < g.n_paths; p += nw) {
        const uint64_t w0 = g.word_off[p], w1 = g.word_off[p + 1] < g.n_words ? g.word_off[p + 1] : g.n_words;
        uint64_t c = 0;
        for (uint64_t w = w0 + lane; w < w1; w += 64) c += (uint64_t)__popcll(g.bitmap[w]);
        c = wave_sum_u64(c);
        if (lane == 0) g.grp_off[p] = c;
    }
}

// after the scan of grp_off: what the host sizes the handle by
__global__ __launch_bounds__(256) void path_contig_counts_kernel(PathArgs g) {
    for (uint32_t ci = blockIdx.x * 256 + threadIdx.x; ci < g.n_contigs; ci += gridDim.x * 256) {
        const uint64_t a = g.path_base[ci], b = g.path_base[ci + 1];
        g.counts[2 * ci] = b - a;
        g.counts[2 * ci + 1] = g.grp_off[b] - g.grp_off[a];
    }
}

__global__ __launch_bounds__(256) void path_fill_kernel(PathArgs g) {
    const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (uint64_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < g.n_paths; p += nw) {
        const uint64_t w0 = g.word_off[p], w1 = g.word_off[p + 1] < g.n_words ? g.word_off[p + 1] : g.n_words;
        const uint32_t lo = g.win_lo[p];
        uint64_t at0 = g.grp_off[p];                                    // wave-uniform: where the next trip's first read goes
        for (uint64_t t = w0; t < w1; t += 64) {
            uint64_t w = t + lane < w1 ? g.bitmap[t + lane] : 0;
            const uint32_t c = (uint32_t)__popcll(w);
            uint32_t inc = c;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t a = __shfl_up(inc, d, 64); if (lane >= d) inc += a; }
            uint64_t at = at0 + (inc - c);
            const uint32_t id0 = lo + (uint32_t)((t + lane - w0) << 6);
            while (w) {
                if (at < g.n_reads_out) g.grp_read[at] = id0 + (uint32_t)__builtin_ctzll(w);
                ++at; w &= w - 1;
            }
            at0 += __shfl(inc, 63, 64);
        }
    }
}

}  // namespace fl
