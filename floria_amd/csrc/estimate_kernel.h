// estimate_kernel.h — the -e / -l estimate (EpsilonEstimator, host/ingest.cpp; file_reader.rs:749-826) on the records of a blob: floria_hip_blob_estimate.
// The function walks the pileup columns (reference positions that lie in the span [pos, end) of at least one record) of all contigs as one sequence and samples a
// column where its running `count` is a multiple of 1000; a sampled column whose depth (bases of M / = / X operations with a query offset below l_seq) is below 5
// does not advance `count`, so its successor is sampled too.  On the ordinal j of covered columns that is a hop chain: from the first j with count = 0 (mod 1000)
// every ordinal up to g(j), the first one >= j with depth >= 5, is sampled, and the next start is g(j) + 1000.
// The kernels work on one WINDOW of positions [w0, w0 + wn) of one contig at a time (memory is linear in wn; the host part walks the windows and carries the state):
//   est_span_kernel      end of every record (once per call)                                       one wavefront per record
//   est_mark_kernel      +1 / -1 into a coverage and a depth difference array                      one wavefront per record, 64 CIGAR operations per trip
//   est_sum_kernel       per chunk of EST_CHUNK positions: the sums of both difference arrays      one workgroup per chunk
//   est_tables_kernel    exclusive scans of the per-chunk tables                                   one workgroup
//   est_depth_kernel     depth and the covered flag per position, covered / first deep per chunk   one workgroup per chunk
//   est_ordinal_kernel   ordinal per position, position per ordinal, next deep position            one workgroup per chunk
//   est_chain_kernel     the hop chain: intervals of sampled ordinals, the new state               one lane
//   est_expand_kernel    intervals -> the ordered list of sampled columns                          one workgroup per interval
//   est_count_kernel     bases of the sampled columns: counts[column][16], rec_hits[record]        one wavefront per record, lanes over the columns in its span
//   est_reduce_kernel    total and most per sampled column                                         one thread per column
// A sampled column is found from a record by binary search in the ordered column list, not through a bitmap: the list is what the chain produces, a record's columns
// are neighbours in it, and one column per 1000 positions would leave a bitmap's words almost all empty.
// BOUNDS: blob reads lie in [cigar_off, cigar_off + 4 n_cigar) and [seq_off, seq_off + (l_seq + 1) / 2), which the host checked against the blob before any launch;
// every end is <= 2^31 - 1 (checked by the host after est_span_kernel), so positions are exact in 64-bit arithmetic.  The per-position arrays are padded to a whole
// number of chunks and every index into them is a position of the window (clipped to [0, wn) before use) or an ordinal below n_cov <= wn; a column index is below
// n_cols, the number the chain counted.  Integer atomics only; LDS: the per-wave tables of 64 operations and the scans' four words; no scratch.
#pragma once
#include "common.h"
#include "wave_util.h"

namespace fl {

constexpr uint32_t EST_WAVES = 4;           // records per workgroup
constexpr uint32_t EST_THREADS = 256;       // threads of a scan workgroup
constexpr uint32_t EST_PER = 8;             // positions per thread
constexpr uint32_t EST_CHUNK = EST_THREADS * EST_PER;
constexpr uint32_t EST_NONE = 0xffffffffu;
constexpr uint32_t EST_PERIOD = 1000, EST_DEEP = 5;
constexpr uint32_t EST_COVERED = 1u << 31;  // ord word: the position is covered; the low 31 bits are its ordinal

struct EstRecs {
    const uint8_t* blob;
    const int32_t* pos;          // [n]
    const uint64_t* cigar_off;   // [n]
    const uint32_t* n_cigar;     // [n]
    const uint64_t* seq_off;     // [n]
    const uint32_t* l_seq;       // [n]
    int64_t* end;                // [n]
    uint32_t* rec_hits;          // [n]
};

struct EstWindow {
    int64_t w0;                  // first position
    uint32_t wn;                 // positions
    uint32_t n_chunks;
    uint32_t* ord;               // [n_chunks * EST_CHUNK] coverage differences (int32), then covered flags, then EST_COVERED | ordinal
    uint32_t* tot;               // [..] depth differences (int32), then the depth
    uint32_t* pos_of_ord;        // [..] position (relative to w0) of every covered ordinal
    uint32_t* next_deep;         // [..] first covered position >= p with depth >= EST_DEEP, or EST_NONE
    int32_t *sum_cov, *sum_dep;  // [n_chunks] per-chunk sums, then their exclusive scans
    int32_t* n_cov;              // [n_chunks] covered positions per chunk, then the exclusive scan
    uint32_t* first_deep;        // [n_chunks] first deep position of the chunk, then of the chunks behind it
};

struct EstState {                // carried on the device from window to window; the host reads it after every chain
    uint64_t count;
    uint32_t n_err, done;
    uint32_t n_cov;              // covered positions of the window
    uint32_t n_iv, n_cols;       // the chain's intervals and the columns in them
    uint32_t overflow;           // the chain met more intervals than the host sized the list for (never, by the sizing rule; the call fails)
};

__device__ __forceinline__ uint32_t est_word(const uint8_t* p) {      // a little-endian word at any alignment
    return (uint32_t)G(p)[0] | (uint32_t)G(p)[1] << 8 | (uint32_t)G(p)[2] << 16 | (uint32_t)G(p)[3] << 24;
}
// M I D N S H P = X: the query is consumed by M I S = X, the reference by M D N = X; a base is given by M = X
__device__ __forceinline__ bool est_q(uint32_t op) { return (0x193u >> op) & 1u; }
__device__ __forceinline__ bool est_r(uint32_t op) { return (0x18du >> op) & 1u; }
__device__ __forceinline__ bool est_base(uint32_t op) { return (0x181u >> op) & 1u; }

// inclusive prefix sums of (iq, ir) over the lanes of a wavefront
__device__ __forceinline__ void est_scan_ops(uint64_t& iq, uint64_t& ir, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t a = __shfl_up((unsigned long long)iq, d, 64), b = __shfl_up((unsigned long long)ir, d, 64);
        if (lane >= d) { iq += a; ir += b; }
    }
}

__global__ __launch_bounds__(64 * EST_WAVES) void est_span_kernel(EstRecs g, uint64_t n) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * EST_WAVES + wv; r < n; r += (uint64_t)gridDim.x * EST_WAVES) {
        const uint32_t n_cig = g.n_cigar[r];
        const uint8_t* const cig = g.blob + g.cigar_off[r];
        uint64_t sum = 0;
        for (uint32_t k = lane; k < n_cig; k += 64) {
            const uint32_t w = est_word(cig + 4 * (uint64_t)k);
            if (est_r(w & 15u)) sum += w >> 4;
        }
        sum = wave_sum_u64(sum);                       // (at most 2^32 operations of less than 2^28 each)
        if (lane == 0) g.end[r] = (int64_t)g.pos[r] + (int64_t)(sum ? sum : 1);
    }
}

// records [lo, hi): the host chose hi so that pos < w0 + wn for every one of them
__global__ __launch_bounds__(64 * EST_WAVES) void est_mark_kernel(EstRecs g, uint64_t lo, uint64_t hi, EstWindow W) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const int64_t w0 = W.w0, w1 = W.w0 + (int64_t)W.wn;
    int* const cov = (int*)W.ord;
    int* const dep = (int*)W.tot;
    for (uint64_t r = lo + (uint64_t)blockIdx.x * EST_WAVES + wv; r < hi; r += (uint64_t)gridDim.x * EST_WAVES) {
        const int64_t pos = g.pos[r], end = g.end[r];
        if (end <= w0 || pos >= w1) continue;
        if (lane == 0) {
            atomicAdd(&cov[(pos > w0 ? pos : w0) - w0], 1);
            if (end < w1) atomicAdd(&cov[end - w0], -1);
        }
        const uint32_t n_cig = g.n_cigar[r];
        const uint64_t l_seq = g.l_seq[r];
        const uint8_t* const cig = g.blob + g.cigar_off[r];
        uint64_t q0 = 0;
        int64_t r0 = pos;
        for (uint32_t k0 = 0; k0 < n_cig && r0 < w1; k0 += 64) {
            const uint32_t k = k0 + lane;
            const uint32_t w = k < n_cig ? est_word(cig + 4 * (uint64_t)k) : 0u;      // (beyond the CIGAR: 0M, consumes nothing)
            const uint32_t op = w & 15u, len = w >> 4;
            uint64_t iq = est_q(op) ? len : 0u, ir = est_r(op) ? len : 0u;
            est_scan_ops(iq, ir, lane);
            if (est_base(op) && len) {
                const uint64_t qs = q0 + iq - len;                                    // the run's first query offset and reference position
                int64_t a = r0 + (int64_t)(ir - len);
                if (qs < l_seq) {
                    const uint64_t room = l_seq - qs;
                    int64_t b = a + (int64_t)(room < len ? room : len);
                    a = a > w0 ? a : w0;
                    b = b < w1 ? b : w1;
                    if (a < b) {
                        atomicAdd(&dep[a - w0], 1);
                        if (b < w1) atomicAdd(&dep[b - w0], -1);
                    }
                }
            }
            q0 += rl64(iq, 63);
            r0 += (int64_t)rl64(ir, 63);
        }
    }
}

struct EstAdd { static constexpr int32_t id = 0; __device__ static int32_t f(int32_t a, int32_t b) { return a + b; } };
struct EstMin { static constexpr int32_t id = -1; __device__ static int32_t f(int32_t a, int32_t b) { return (uint32_t)a < (uint32_t)b ? a : b; } };      // unsigned minimum, EST_NONE neutral
// The combination of v over the threads in front of this one (REV: behind it) of an EST_THREADS workgroup, and over all of them; s: four words of LDS.
template <class Op, bool REV>
__device__ __forceinline__ int32_t est_block_scan(int32_t v, int32_t* s, int32_t& all) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    int32_t ex = Op::id, inc = v;                     // ex: the lanes in front (behind), inc: ex and this lane
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int32_t a = REV ? __shfl_down(inc, d, 64) : __shfl_up(inc, d, 64);
        if (REV ? lane + d < 64 : lane >= d) inc = Op::f(inc, a);
    }
    {
        const int32_t a = REV ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
        if (REV ? lane < 63 : lane > 0) ex = a;
    }
    if (lane == (REV ? 0u : 63u)) s[wv] = inc;
    __syncthreads();
    int32_t t = Op::id;
    all = Op::id;
#pragma unroll
    for (uint32_t i = 0; i < EST_THREADS / 64; ++i) {
        const int32_t x = s[i];
        if (REV ? i > wv : i < wv) t = Op::f(t, x);
        all = Op::f(all, x);
    }
    __syncthreads();
    return Op::f(t, ex);
}

__global__ __launch_bounds__(EST_THREADS) void est_sum_kernel(EstWindow W) {
    __shared__ int32_t s[EST_THREADS / 64];
    for (uint32_t c = blockIdx.x; c < W.n_chunks; c += gridDim.x) {
        const uint64_t p = (uint64_t)c * EST_CHUNK + threadIdx.x * EST_PER;
        const int4 a0 = *(const int4*)(W.ord + p), a1 = *(const int4*)(W.ord + p + 4), b0 = *(const int4*)(W.tot + p), b1 = *(const int4*)(W.tot + p + 4);
        int32_t sc, sd;
        (void)est_block_scan<EstAdd, false>(a0.x + a0.y + a0.z + a0.w + a1.x + a1.y + a1.z + a1.w, s, sc);
        (void)est_block_scan<EstAdd, false>(b0.x + b0.y + b0.z + b0.w + b1.x + b1.y + b1.z + b1.w, s, sd);
        if (threadIdx.x == 0) { W.sum_cov[c] = sc; W.sum_dep[c] = sd; }
    }
}

// one workgroup: a and b (each may be null) become their exclusive prefix sums, m its exclusive suffix minimum; n_cov (may be null) receives the sum of a
__global__ __launch_bounds__(EST_THREADS) void est_tables_kernel(int32_t* a, int32_t* b, uint32_t* m, uint32_t n, uint32_t* n_cov) {
    __shared__ int32_t s[EST_THREADS / 64];
    int32_t ca = 0, cb = 0, cm = -1;
    for (uint32_t i0 = 0; i0 < n; i0 += EST_THREADS) {
        const uint32_t i = i0 + threadIdx.x, ri = n - 1u - i;      // (ri is used only where i < n)
        const bool in = i < n;
        int32_t all;
        if (a) { const int32_t v = in ? a[i] : 0; const int32_t ex = est_block_scan<EstAdd, false>(v, s, all); if (in) a[i] = ca + ex; ca += all; }
        if (b) { const int32_t v = in ? b[i] : 0; const int32_t ex = est_block_scan<EstAdd, false>(v, s, all); if (in) b[i] = cb + ex; cb += all; }
        if (m) {                                                   // from the table's end: thread t takes entry n - 1 - (i0 + t), so "in front" is "behind"
            const int32_t v = in ? (int32_t)m[ri] : -1;
            const int32_t ex = est_block_scan<EstMin, false>(v, s, all);
            if (in) m[ri] = (uint32_t)EstMin::f(cm, ex);
            cm = EstMin::f(cm, all);
        }
    }
    if (n_cov && threadIdx.x == 0) *n_cov = (uint32_t)ca;
}

__global__ __launch_bounds__(EST_THREADS) void est_depth_kernel(EstWindow W) {
    __shared__ int32_t s[EST_THREADS / 64];
    for (uint32_t c = blockIdx.x; c < W.n_chunks; c += gridDim.x) {
        const uint64_t p = (uint64_t)c * EST_CHUNK + threadIdx.x * EST_PER;
        const int4 a0 = *(const int4*)(W.ord + p), a1 = *(const int4*)(W.ord + p + 4), b0 = *(const int4*)(W.tot + p), b1 = *(const int4*)(W.tot + p + 4);
        int32_t cv[EST_PER] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, dp[EST_PER] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (uint32_t i = 1; i < EST_PER; ++i) { cv[i] += cv[i - 1]; dp[i] += dp[i - 1]; }
        int32_t all;
        const int32_t bc = W.sum_cov[c] + est_block_scan<EstAdd, false>(cv[EST_PER - 1], s, all);
        const int32_t bd = W.sum_dep[c] + est_block_scan<EstAdd, false>(dp[EST_PER - 1], s, all);
        uint32_t n = 0, first = EST_NONE;
#pragma unroll
        for (uint32_t i = 0; i < EST_PER; ++i) {
            const bool covered = p + i < W.wn && bc + cv[i] > 0;
            dp[i] += bd;
            cv[i] = covered;
            n += covered;
            if (covered && (uint32_t)dp[i] >= EST_DEEP && first == EST_NONE) first = (uint32_t)(p + i);
        }
        *(int4*)(W.ord + p) = make_int4(cv[0], cv[1], cv[2], cv[3]); *(int4*)(W.ord + p + 4) = make_int4(cv[4], cv[5], cv[6], cv[7]);
        *(int4*)(W.tot + p) = make_int4(dp[0], dp[1], dp[2], dp[3]); *(int4*)(W.tot + p + 4) = make_int4(dp[4], dp[5], dp[6], dp[7]);
        int32_t cn, cf;
        (void)est_block_scan<EstAdd, false>((int32_t)n, s, cn);
        (void)est_block_scan<EstMin, false>((int32_t)first, s, cf);
        if (threadIdx.x == 0) { W.n_cov[c] = cn; W.first_deep[c] = (uint32_t)cf; }
    }
}

__global__ __launch_bounds__(EST_THREADS) void est_ordinal_kernel(EstWindow W) {
    __shared__ int32_t s[EST_THREADS / 64];
    for (uint32_t c = blockIdx.x; c < W.n_chunks; c += gridDim.x) {
        const uint64_t p = (uint64_t)c * EST_CHUNK + threadIdx.x * EST_PER;
        const int4 a0 = *(const int4*)(W.ord + p), a1 = *(const int4*)(W.ord + p + 4), b0 = *(const int4*)(W.tot + p), b1 = *(const int4*)(W.tot + p + 4);
        const int32_t cv[EST_PER] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, dp[EST_PER] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        uint32_t n = 0, first = EST_NONE;
#pragma unroll
        for (uint32_t i = 0; i < EST_PER; ++i) {
            n += (uint32_t)cv[i];
            if (cv[i] && (uint32_t)dp[i] >= EST_DEEP && first == EST_NONE) first = (uint32_t)(p + i);
        }
        int32_t all;
        uint32_t o = (uint32_t)(W.n_cov[c] + est_block_scan<EstAdd, false>((int32_t)n, s, all));
        uint32_t nd = (uint32_t)EstMin::f((int32_t)W.first_deep[c], est_block_scan<EstMin, true>((int32_t)first, s, all));      // the first deep position behind this thread's
        uint32_t ow[EST_PER], nw[EST_PER];
#pragma unroll
        for (uint32_t i = 0; i < EST_PER; ++i) {
            ow[i] = cv[i] ? (EST_COVERED | o) : o;
            if (cv[i]) { W.pos_of_ord[o] = (uint32_t)(p + i); ++o; }      // o < the window's covered positions <= wn
        }
#pragma unroll
        for (uint32_t i = EST_PER; i-- > 0;) {
            if (cv[i] && (uint32_t)dp[i] >= EST_DEEP) nd = (uint32_t)(p + i);
            nw[i] = nd;
        }
        *(uint4*)(W.ord + p) = make_uint4(ow[0], ow[1], ow[2], ow[3]); *(uint4*)(W.ord + p + 4) = make_uint4(ow[4], ow[5], ow[6], ow[7]);
        *(uint4*)(W.next_deep + p) = make_uint4(nw[0], nw[1], nw[2], nw[3]); *(uint4*)(W.next_deep + p + 4) = make_uint4(nw[4], nw[5], nw[6], nw[7]);
    }
}

// One lane walks the hops: at most stop deep columns, and one interval (first ordinal, last ordinal, first column) for each of them and the shallow run in front.
__global__ __launch_bounds__(64) void est_chain_kernel(EstState* st, uint32_t stop, EstWindow W, uint32_t* iv, uint32_t max_iv) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t count = st->count;
    uint32_t n_err = st->n_err, done = 0, n_iv = 0, n_cols = 0, cur = 0, overflow = 0;
    const uint32_t n_cov = st->n_cov;
    for (;;) {
        const uint32_t rem = (uint32_t)(count % EST_PERIOD), skip = rem ? EST_PERIOD - rem : 0u;
        if (skip >= n_cov - cur) { count += n_cov - cur; break; }
        const uint32_t j = cur + skip;
        count += skip;
        const uint32_t deep = W.next_deep[W.pos_of_ord[j]];
        const uint32_t last = deep == EST_NONE ? n_cov - 1u : (W.ord[deep] & ~EST_COVERED);
        if (n_iv < max_iv) { iv[3 * n_iv] = j; iv[3 * n_iv + 1] = last; iv[3 * n_iv + 2] = n_cols; } else overflow = 1;
        ++n_iv;
        n_cols += last - j + 1u;
        if (deep == EST_NONE) break;                  // shallow to the window's end: count stays where it is, the next window's first column is sampled
        if (++n_err >= stop) { done = 1; break; }
        ++count;
        cur = last + 1u;
    }
    st->count = count; st->n_err = n_err; st->done = done; st->n_iv = n_iv; st->n_cols = n_cols; st->overflow = overflow;
}

__global__ __launch_bounds__(EST_THREADS) void est_expand_kernel(const uint32_t* iv, uint32_t n_iv, const uint32_t* pos_of_ord, uint32_t* col_pos) {
    for (uint32_t i = blockIdx.x; i < n_iv; i += gridDim.x) {
        const uint32_t j0 = iv[3 * i], n = iv[3 * i + 1] - j0 + 1u, c0 = iv[3 * i + 2];
        for (uint32_t k = threadIdx.x; k < n; k += EST_THREADS) col_pos[c0 + k] = pos_of_ord[j0 + k];
    }
}

__global__ __launch_bounds__(64 * EST_WAVES) void est_count_kernel(EstRecs g, uint64_t lo, uint64_t hi, int64_t w0, uint32_t wn, const uint32_t* col_pos, uint32_t n_cols, uint32_t* counts) {
    __shared__ uint64_t s_rend[EST_WAVES][64], s_qend[EST_WAVES][64];
    __shared__ uint32_t s_word[EST_WAVES][64];
    const uint32_t lane = threadIdx.x & 63u, wv = uni(threadIdx.x >> 6);
    uint64_t* const rend = s_rend[wv];
    uint64_t* const qend = s_qend[wv];
    uint32_t* const word = s_word[wv];
    const int64_t w1 = w0 + (int64_t)wn;
    for (uint64_t r = lo + (uint64_t)blockIdx.x * EST_WAVES + wv; r < hi; r += (uint64_t)gridDim.x * EST_WAVES) {
        const int64_t pos = g.pos[r], end = g.end[r];
        if (end <= w0 || pos >= w1) continue;
        const uint32_t a = (uint32_t)((pos > w0 ? pos : w0) - w0), b = (uint32_t)((end < w1 ? end : w1) - w0);      // the record's columns lie in [a, b)
        uint32_t c = 0;                                   // the first column at or behind a (the same search in every lane)
        for (uint32_t top = n_cols; c < top;) { const uint32_t mid = c + (top - c) / 2; if (col_pos[mid] < a) c = mid + 1; else top = mid; }
        if (c >= n_cols || col_pos[c] >= b) continue;
        const uint32_t n_cig = g.n_cigar[r];
        const uint64_t l_seq = g.l_seq[r];
        const uint8_t* const cig = g.blob + g.cigar_off[r];
        const uint8_t* const seq = g.blob + g.seq_off[r];
        uint64_t q0 = 0;
        int64_t r0 = pos;
        uint32_t hits = 0;
        for (uint32_t k0 = 0; k0 < n_cig; k0 += 64) {
            const uint32_t k = k0 + lane;
            const uint32_t w = k < n_cig ? est_word(cig + 4 * (uint64_t)k) : 0u;
            const uint32_t op = w & 15u, len = w >> 4;
            uint64_t iq = est_q(op) ? len : 0u, ir = est_r(op) ? len : 0u;
            est_scan_ops(iq, ir, lane);
            const uint64_t tq = rl64(iq, 63), tr = rl64(ir, 63);
            if (tr != 0) {
                rend[lane] = ir; qend[lane] = iq; word[lane] = w;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (;;) {                                // the columns inside this trip's reference range, 64 at a time (every column at c and behind is >= r0)
                    const uint32_t idx = c + lane;
                    uint64_t d = 0;
                    bool in = false;
                    if (idx < n_cols) { d = (uint64_t)(w0 + (int64_t)col_pos[idx] - r0); in = d < tr; }
                    const uint32_t n_in = (uint32_t)__popcll(__ballot(in));
                    if (n_in == 0) break;
                    if (in) {
                        uint32_t j = 0;                   // the first operation whose reference end lies above the column
#pragma unroll
                        for (uint32_t t = 32; t > 0; t >>= 1) if (rend[j + t - 1] <= d) j += t;
                        const uint32_t wj = word[j], lenj = wj >> 4;
                        if (est_base(wj & 15u)) {
                            const uint64_t sp = q0 + (qend[j] - lenj) + (d - (rend[j] - lenj));
                            if (sp < l_seq) {
                                const uint32_t byte = G(seq)[sp >> 1];
                                atomicAdd(&counts[(uint64_t)idx * 16 + (sp & 1u ? byte & 15u : byte >> 4)], 1u);
                                ++hits;
                            }
                        }
                    }
                    c += n_in;
                }
                __builtin_amdgcn_wave_barrier();         // (the next trip rewrites the tables)
            }
            q0 += tq;
            r0 += (int64_t)tr;
            if (c >= n_cols || col_pos[c] >= b) break;
        }
        hits = wave_sum_u32(hits);
        if (lane == 0 && hits) atomicAdd(&g.rec_hits[r], hits);
    }
}

__global__ __launch_bounds__(EST_THREADS) void est_reduce_kernel(const uint32_t* counts, uint32_t n_cols, uint32_t* col_total, uint32_t* col_most) {
    for (uint32_t c = blockIdx.x * EST_THREADS + threadIdx.x; c < n_cols; c += gridDim.x * EST_THREADS) {
        uint32_t total = 0, most = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint4 v = *(const uint4*)(counts + (uint64_t)c * 16 + 4 * i);
            total += v.x + v.y + v.z + v.w;
            most = max(max(most, max(v.x, v.y)), max(v.z, v.w));
        }
        col_total[c] = total; col_most[c] = most;
    }
}

}  // namespace fl
