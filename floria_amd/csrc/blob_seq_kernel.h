// blob_seq_kernel.h — the bases and qualities of many records of a blob as the read writers want them (floria_hip_blob_sequences): what frag_sequences
// (host/ingest.cpp) makes of a host record, for every record of one ingest round in one call.
//   base     the 4-bit code 1 / 2 / 4 / 8 is 'A' / 'C' / 'G' / 'T', every other code 'A' (the reference writes 'A' for whatever is no ACGT)
//   quality  q > 222 ? 255 : q + 33   (checked_add(33).unwrap_or(255))
// One wavefront per record, four records per workgroup, in a grid that strides over the records.  Record r owns bytes [base_off[r], base_off[r] + l_seq[r]) of both
// outputs.  The lanes stride over GROUPS of eight output bytes that start on an 8-byte boundary of the output: a lane reads the group's four packed bytes (five where
// the group begins on a low nibble: the output's alignment, not the input's, decides where a group begins, and then neighbouring groups share one byte) and its eight
// quality bytes by byte loads — the offsets into the blob are arbitrary — and writes each output as one 8-byte store.  The up to seven bytes in front of the first
// boundary and behind the last whole group are written one per lane.  For an odd l_seq the low nibble of the last packed byte is padding: no base index reaches it.
// BOUNDS: every read lies in [seq_off, seq_off + (l_seq + 1) / 2) or [qual_off, qual_off + l_seq), which the host has checked against the blob's length before the
// launch; every write lies in the record's own output range.  No LDS, no scratch.
#pragma once
#include "common.h"

namespace fl {

constexpr uint32_t SEQ_WAVES = 4;      // records per workgroup

struct BlobSeqArgs {
    const uint8_t* blob;
    const uint64_t *seq_off, *qual_off;      // [n]
    const uint32_t* l_seq;                   // [n]
    const uint64_t* base_off;                // [n + 1] prefix sums of l_seq
    uint8_t *bases, *quals;                  // [base_off[n]] each, 8-byte aligned
    uint64_t n;
};

__host__ __device__ __forceinline__ uint32_t seq_letter(uint32_t code) { return code == 2 ? 'C' : code == 4 ? 'G' : code == 8 ? 'T' : 'A'; }
__host__ __device__ __forceinline__ uint32_t seq_qual(uint32_t q) { return q > 222 ? 255u : q + 33u; }

__global__ __launch_bounds__(64 * SEQ_WAVES) void blob_seq_kernel(BlobSeqArgs g) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * SEQ_WAVES + wave; r < g.n; r += (uint64_t)gridDim.x * SEQ_WAVES) {
        const uint32_t len = g.l_seq[r];
        const uint64_t so = g.seq_off[r], qo = g.qual_off[r], bo = g.base_off[r];
        const uint32_t to_boundary = (uint32_t)((8 - (bo & 7)) & 7), head = to_boundary < len ? to_boundary : len;
        const uint32_t groups = (len - head) >> 3, tail = head + 8 * groups;
        // lanes 0..6: the bytes in front of the first boundary; lanes 8..14: the bytes behind the last whole group
        const uint32_t k = lane < 8 ? lane : tail + (lane - 8);
        if (lane < 8 ? lane < head : (lane < 16 && k < len)) {
            const uint32_t b = G(g.blob)[so + (k >> 1)];
            g.bases[bo + k] = (uint8_t)seq_letter(k & 1u ? b & 15u : b >> 4);
            g.quals[bo + k] = (uint8_t)seq_qual(G(g.blob)[qo + k]);
        }
        for (uint32_t gi = lane; gi < groups; gi += 64) {
            const uint32_t j = head + 8 * gi, low = j & 1u;      // bases j .. j + 7; `low`: base j is the low nibble of its byte
            const uint64_t s = so + (j >> 1);
            // ten nibbles, the first in bits 36..39; base j + t is nibble t + low (the fifth byte holds base j + 7 where `low`, and is not read otherwise)
            uint64_t v = (uint64_t)G(g.blob)[s] << 32 | (uint64_t)G(g.blob)[s + 1] << 24 | (uint64_t)G(g.blob)[s + 2] << 16 | (uint64_t)G(g.blob)[s + 3] << 8;
            if (low) v |= G(g.blob)[s + 4];
            v <<= 4 * low;                                       // base j + t is now nibble t: bits 36 - 4t .. 39 - 4t
            uint32_t w0 = 0, w1 = 0, q0 = 0, q1 = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                w0 |= seq_letter((uint32_t)(v >> (36 - 4 * t)) & 15u) << (8 * t);
                w1 |= seq_letter((uint32_t)(v >> (20 - 4 * t)) & 15u) << (8 * t);
                q0 |= seq_qual(G(g.blob)[qo + j + t]) << (8 * t);
                q1 |= seq_qual(G(g.blob)[qo + j + 4 + t]) << (8 * t);
            }
            *(uint2*)(g.bases + bo + j) = make_uint2(w0, w1);   // bo + j is a multiple of 8
            *(uint2*)(g.quals + bo + j) = make_uint2(q0, q1);
        }
    }
}

}  // namespace fl
