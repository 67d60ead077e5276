// span_kernel.h — the two lookups write_reads (file_writer.rs:460-530) makes in Frag::snp_pos_to_seq_pos per (haploset, read), on resident contigs that carry
// positions (floria_hip_read_spans): the SEQ_POS word (`mate << 31 | seq_pos`) of the read's first cell at or behind the haploset's left end and of its last cell
// at or before its right end.  The groups are those of floria_hip_haploset_alleles: reads of a contig plus an inclusive 1-based SNP range [lo, hi].
//
// One thread per entry j of grp_read.  The entry's group is found by a binary search in grp_off (the last g with grp_off[g] <= j < grp_off[g + 1]: empty groups
// are stepped over by the search itself), the read's ascending SNP slice comes from read_off, two binary searches give the lower bound of lo and the upper bound
// of hi, and one load each from the position region gives the answers.  The two are answered independently: a group with hi < lo is no special case.
// No LDS, no scratch, no atomics, nothing shared between threads.
// Every index is compared with a length the host validated before the launch (n_groups, n_contigs, the contig's n_reads and n_cells) before it addresses
// anything; an entry that fails such a comparison (the host refuses those calls: this is the second line) gets SPAN_NONE twice.
#pragma once
#include "common.h"

namespace fl {

constexpr uint32_t SPAN_NONE = 0xffffffffu;

struct SpanContig {
    const uint32_t* read_off;      // [n_reads + 1]
    const uint32_t* snp;           // [n_cells] ascending inside a read
    const uint32_t* seq_pos;       // [n_cells] the SEQ_POS words
    uint32_t n_reads, n_cells;
};

struct SpanArgs {
    const SpanContig* contigs;     // [n_contigs]
    const uint32_t* grp_contig;    // [n_groups]
    const uint64_t* grp_off;       // [n_groups + 1] ascending from 0
    const uint32_t* grp_read;      // [n_entries]
    const uint32_t* grp_range;     // [2 * n_groups] lo, hi (1-based, inclusive)
    uint32_t* left;                // [n_entries]
    uint32_t* right;               // [n_entries]
    uint64_t n_entries;
    uint32_t n_groups, n_contigs;
};

__global__ __launch_bounds__(256) void read_spans_kernel(SpanArgs g) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n_entries) return;
    uint32_t a = 0, z = g.n_groups;                         // the group of entry j: the number of g in [1, n_groups] with grp_off[g] <= j
    while (a < z) { const uint32_t mid = a + ((z - a) >> 1); if (g.grp_off[mid + 1] <= j) a = mid + 1; else z = mid; }
    uint32_t L = SPAN_NONE, R = SPAN_NONE;
    const uint32_t ci = a < g.n_groups ? g.grp_contig[a] : g.n_contigs;
    if (ci < g.n_contigs) {
        const SpanContig cd = g.contigs[ci];
        const uint32_t r = g.grp_read[j];
        if (r < cd.n_reads) {
            const uint32_t lo = g.grp_range[2 * (uint64_t)a], hi = g.grp_range[2 * (uint64_t)a + 1];
            uint32_t b = G(cd.read_off)[r], e = G(cd.read_off)[r + 1];
            e = e > cd.n_cells ? cd.n_cells : e;
            b = b > e ? e : b;
            uint32_t x = b, y = e;                          // first cell with snp >= lo
            while (x < y) { const uint32_t mid = x + ((y - x) >> 1); if (G(cd.snp)[mid] < lo) x = mid + 1; else y = mid; }
            if (x < e) L = G(cd.seq_pos)[x];
            x = b; y = e;                                   // first cell with snp > hi: the one before it is the last with snp <= hi
            while (x < y) { const uint32_t mid = x + ((y - x) >> 1); if (G(cd.snp)[mid] <= hi) x = mid + 1; else y = mid; }
            if (x > b) R = G(cd.seq_pos)[x - 1];
        }
    }
    g.left[j] = L; g.right[j] = R;
}

}  // namespace fl
