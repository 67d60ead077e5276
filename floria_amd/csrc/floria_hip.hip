// floria_hip.hip — host side of libfloria_hip.so (C ABI in include/floria_hip.h) + kernel launches.
//
// Host responsibilities (the reference does these on its rayon workers / main thread):
//   get_range_with_lengths            utils_frags.rs:405-463      -> floria_hip_block_ranges
//   find_reads_in_interval            local_clustering.rs:12-59   -> build_block_lists (binary search + filter)
//   per-ploidy loop of get_local_hap_blocks graph_processing.rs:132-252 -> one launch triple per ploidy:
//       beam_kernel -> optimize_kernel -> select_kernel (the stop rule sets blk_done so later
//       ploidies skip finished blocks: no speculative work, results identical)
//   separate_broken_haplogroups / sort_parts  part_block_manip.rs:27-98,276-288 -> host bookkeeping after
//       reassign_kernel (floria_hip_reassign_batch), or haploset_kernel.h's kernels behind it (floria_hip_reassign_batch_resident: the result stays on the device)
// There is NO CPU compute fallback: every entry point needs a working HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <utility>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/floria_hip.h"
#include "beam_kernel.h"
#include "wave_util.h"
#include "beam_slab_kernel.h"
#include "beam_wide_kernel.h"
#include "optimize_kernel.h"
#include "reassign_kernel.h"
#include "hapq_kernel.h"
#include "blocks_kernel.h"
#include "graph_kernel.h"
#include "stats_kernel.h"
#include "realign_kernel.h"
#include "realign_walk_kernel.h"
#include "pileup_kernel.h"
#include "realign_gather_kernel.h"
#include "upload_kernel.h"
#include "assemble_kernel.h"
#include "assemble_order_kernel.h"
#include "mono_kernel.h"
#include "span_kernel.h"
#include "haploset_kernel.h"
#include "path_kernel.h"
#include "inflate_kernel.h"
#include "blob_seq_kernel.h"
#include "estimate_kernel.h"

static_assert(FLORIA_MAX_PLOIDY == fl::MAX_PLOIDY, "ploidy limits out of sync");

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

// HIPCHK_AS: the message is `prefix` + the error string ("assemble: ", "contig upload: ", ...); HIPCHK: the expression's own text is the prefix.  Both RETURN, so
// whatever a function owns by then (an arena, a result, handles) is released by a guard object, never by hand.
#define HIPCHK_AS(prefix, expr)                                                                        \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(_e == hipErrorOutOfMemory ? FLORIA_E_NOMEM : FLORIA_E_DEVICE,                  \
                        std::string(prefix) + hipGetErrorString(_e));                                  \
    } while (0)
#define HIPCHK(expr) HIPCHK_AS(#expr ": ", expr)

constexpr double DIV_FACTOR  = 0.25;   // constants.rs:5
constexpr double PROB_CUTOFF = 0.01;   // constants.rs:6
constexpr uint32_t BINOM_NMAX_CAP = 1024;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(FLORIA_E_NOMEM, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// A call's device arrays, carved out of one scratch buffer: segments in the order they are asked for, each starting on a 256-B boundary.
struct Seg { size_t off, bytes; };
struct Carve {
    size_t cursor = 0;
    char* base = nullptr;
    Seg seg(size_t bytes) { const Seg s{cursor, bytes}; cursor += (bytes + 255) & ~(size_t)255; return s; }
    int place(DevBuf& buf) { const int rc = buf.ensure(cursor + 256); base = buf.as<char>(); return rc; }      // (after the last seg())
    template <class T = void> T* at(Seg s) const { return (T*)(base + s.off); }
    hipError_t up(Seg s, const void* src, size_t bytes, hipStream_t st) const { return bytes ? hipMemcpyAsync(base + s.off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; }
};

// Pinned, device-mapped host memory for the small latency-critical transfers of a call (block counts down, offsets and job lists up): kernels read and
// write it directly.  A hipMemcpyAsync of a few KB shares the SDMA queues with the pileup's bulk upload and was seen waiting behind all of it
// (block counts on the host after 14.7 ms instead of 4.3 ms in two calls out of three).
struct HostBox {
    char* h = nullptr;       // host address
    char* d = nullptr;       // the same bytes as the device sees them
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc((void**)&h, want, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d, h, 0);
        if (e != hipSuccess) { if (h) (void)hipHostFree(h); h = nullptr; d = nullptr; return fail(FLORIA_E_NOMEM, std::string("hipHostMalloc(mapped, ") + std::to_string(want) + "): " + hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release() { if (h) (void)hipHostFree(h); h = nullptr; d = nullptr; cap = 0; }
};

// Pageable sources go through a ring of pinned staging buffers filled by a few host threads (a single pageable hipMemcpy is
// staged by the runtime on one thread at a few GB/s); pinned sources are handed to the DMA engine as they are.
struct StagePool {
    static constexpr size_t SEG = 16u << 20;      // large pieces: every copy in a stream pays ~0.2 ms of completion-signal latency
    static constexpr uint32_t NBUF = 8;
    char* buf[NBUF] = {};
    hipEvent_t ev[NBUF] = {};
    bool used[NBUF] = {};
    int init() {
        for (uint32_t i = 0; i < NBUF; ++i) if (!buf[i]) {
            if (hipHostMalloc((void**)&buf[i], SEG, hipHostMallocDefault) != hipSuccess) return fail(FLORIA_E_NOMEM, "hipHostMalloc(staging) failed");
            if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return fail(FLORIA_E_DEVICE, "hipEventCreate failed");
        }
        return 0;
    }
    void release() { for (uint32_t i = 0; i < NBUF; ++i) { if (buf[i]) (void)hipHostFree(buf[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); buf[i] = nullptr; ev[i] = nullptr; used[i] = false; } }
};

uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

// Large result arrays (read ids, partitions: tens of MB per S1 call) come from a small process-wide cache: a fresh malloc of
// that size is an mmap whose pages fault one by one under the device->host copy.  Header = capacity, 64 B before the payload.
namespace {
struct BigCache {
    std::mutex m;
    std::vector<std::pair<void*, size_t>> v;      // (base, capacity)
    void* get(size_t n) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].second >= n && v[i].second <= 2 * n + 4096) { void* b = v[i].first; v.erase(v.begin() + i); return (char*)b + 64; }
        }
        void* b = malloc(n + 64);
        if (!b) return nullptr;
        *(size_t*)b = n;
        return (char*)b + 64;
    }
    void put(void* payload) {
        if (!payload) return;
        void* b = (char*)payload - 64;
        const size_t cap = *(size_t*)b;
        std::lock_guard<std::mutex> l(m);
        if (cap >= (1u << 20) && v.size() < 8) v.push_back({b, cap}); else free(b);
    }
};
BigCache g_big;
}  // namespace

// Tuning / test knobs of a context (floria_hip_set_option); the defaults are what bench.py measures.  Read from the environment
// ONCE, at floria_hip_create (FLORIA_HIP_GROUPS, FLORIA_HIP_BEAM=generic|slab|wide, FLORIA_HIP_NO_SPECIALIZED, FLORIA_HIP_NO_P1_SHORTCUT,
// FLORIA_HIP_OPT_THREADS, FLORIA_HIP_OPT_GLOBAL, FLORIA_HIP_SPECULATE, FLORIA_HIP_FUSE_P1); none of them changes results.
struct Knobs {
    uint32_t groups = 0;          // job groups (0 = auto: 2 when the batch has >= 48 x CUs non-empty blocks)
    uint32_t beam_path = 0;       // 0 auto | 1 generic | 2 slab | 3 wide
    uint32_t no_specialized = 0;  // runtime ploidy / beam width instead of the template instances
    uint32_t no_p1_shortcut = 0;  // run the beam kernel for ploidy 1 too
    uint32_t opt_threads = 0;     // 0 auto | 128 | 512 | 1024
    uint32_t opt_global = 0;      // optimise histogram in HBM
    int32_t  speculate = -1;      // ploidy stages: -1 auto | 0 one ploidy per stage | 1 all ploidies at once | 2 {1,2,3} then {4..P}
    uint32_t upload_chunks = 0;   // floria_hip_phase_pileups_batch: chunks the cell arrays travel in (0 = auto by size, <= 8)
    uint32_t trace = 0;           // print host-side timestamps of the S1 call to stderr
    uint32_t spec_gate_div = 2;   // speculative stages: grid of the gated (ploidy >= 4) beam launches = slots / this
    uint32_t reassign_path = 0;   // S2 kernel: 0 auto | 1 workgroup-parallel | 2 one-wavefront chain
    uint32_t no_bulk = 0;         // (tests) beam_slab_kernel: every step through the general insert path (entry table, duplicate test, evictions)
    uint32_t fx_tags = 0;         // (A/B) reference arithmetic: cap on the words of a position map's claim table (0 = as many as cost no workgroup per CU)
    uint32_t arith_ow6 = 0;       // (A/B) ... the optimise kernel compiled for six waves per SIMD at every ploidy
    uint32_t asm_order_general = 0;      // (tests) floria_hip_assemble_contigs_ordered: every fragment's set order through the general kernel (assemble_order_kernel.h)
    uint32_t chain_wgs = 0;       // (tests) the grid-stride launches of the resident chain (walk, realign gather / scatter, assemble, assemble order, mono FILL / ORDER) use at most this
                                  // many workgroups, and the general order kernel this many threads: a wavefront's second trip at small shapes (0 = the grids as they are)
    uint32_t arith_replay = 0;    // (tests) reference arithmetic: replay every position map insertion by insertion (the home-bucket rule of optimize_kernel.h off)
    uint32_t arith_hbm = 0;       // (tests) reference arithmetic: position-map tables and first-insertion keys in HBM scratch even where they fit into LDS
    uint32_t opt_block_order = 0; // (A/B, tests) optimise: the build / distance passes visit the reads in block order instead of longest first
    uint32_t s1_no_lists = 0;     // floria_hip_phase_*: the read-id lists and partition bytes stay on the device (read_id / part of the result are NULL): for a host that joins paths there (floria_hip_join_paths)
    uint32_t s2_assign_only = 0;  // S2 returns the haplogroups as re-inserted (input order): separate_broken_haplogroups and sort_parts are left to a host that iterates its own sets
    uint32_t arith = 0;           // 1 = the reference's own running f64 sums in its own orders (arith_kernel.h; slower kernels), 0 = the canonical (Q24, #eps) form
    int32_t  tail_overlap = 0;    // one ploidy per stage: the LAST ploidy's beam launch runs beside the optimise launch of the ploidy below, every job waiting for its block's
                                  // stop rule (run_phase): 0 off (default: measured level) | 1 on
    uint32_t tail_waves = 2;      // ... with this many waves per CU
    uint32_t opt_packed = 1;      // optimise: the build / distance passes stream the 4-byte packed cells (ContigDev::cell_pk) with 16-byte loads where every contig of the call has
                                  // them and the plan takes a 512-thread ploidy-specialised instance (plan_ploidies); 0 = the 8-byte cells (cell_snp + cell_aw)
    uint32_t opt_delta = 1;       // optimise, canonical ploidy-specialised instances of 512 threads: distances kept as exact packed integers, and behind an accepted round only the terms at the flipped
                                  // (position, partition) code bytes are exchanged (optimize_kernel.h: the delta pass); 0 = f64 slots and the interval pass every time
    int32_t  fuse_p1 = -1;        // one ploidy per stage, canonical arithmetic, max_ploidy >= 2, ploidy-1 shortcut on: ploidy 1 has no launch of its own, the ploidy-2 optimise job
                                  // computes it from its own histogram (optimize_kernel.h, with_p1): -1 auto (on where eligible) | 0 off | 1 on where eligible
};

struct Arena;

struct floria_hip_ctx {
    int device = 0;
    uint32_t hw_queues = 0;                   // streams that really run side by side on this device (probe_hw_queues at create)
    hipStream_t stream = nullptr;
    uint32_t user_slots = 0;
    Knobs knobs;
    int n_cu = 256;
    // launch lanes (job group x position inside a ploidy stage): every lane has its own stream and scratch slice, see size_scratch / lane_streams
    static constexpr uint32_t MAX_GROUPS = 8;
    static constexpr uint32_t MAX_LANES = 32;
    hipStream_t gstream[MAX_LANES] = {};
    hipStream_t gstream_low[MAX_LANES] = {};      // speculative stages: the lanes of ploidy >= 4 (dispatched after the ploidies every block needs)
    hipEvent_t ev_fork[MAX_LANES] = {}, ev_join[MAX_LANES] = {};
    hipEvent_t ev_gate[MAX_GROUPS] = {};       // speculative stages: the beam search of ploidy 2 of group g has finished (ploidies >= 4 start behind it)
    hipStream_t tstream[MAX_GROUPS] = {};      // the last ploidy's beam launch of group g when it runs beside the optimise launch below it (Knobs::tail_overlap)
    hipEvent_t ev_tail[MAX_GROUPS] = {}, ev_tail_join[MAX_GROUPS] = {};
    hipStream_t copy_stream = nullptr;        // read-id lists go back to the host while the launch loop runs
    hipEvent_t ev_rids = nullptr;
    hipEvent_t ev_chunk[MAX_GROUPS + 1] = {};  // floria_hip_phase_pileups_batch: chunk g of the cell arrays has landed and is flattened
    hipEvent_t ev_copied[MAX_GROUPS + 1] = {}; //   ... has landed (the flatten launches run on their own stream, so the DMA queue never waits for a kernel)
    hipStream_t flat_stream = nullptr;
    HostBox box;                              // s1_core's small transfers
    // cached tables
    double binom_eps = -1.0;
    uint32_t binom_nmax = 0;
    DevBuf d_binom;
    DevBuf d_hash;            // Rq1 | Rp1 | Rq2 | Rp2, each hash_len u64
    uint32_t hash_len = 0;
    uint32_t w24[256];
    DevBuf d_w24;             // the same table on the device (flatten_kernel)
    uint64_t Rk1[FLORIA_MAX_PLOIDY], Rk2[FLORIA_MAX_PLOIDY];
    // scratch pools
    DevBuf state_pool, hist_pool, opt_hist, opt_dist, opt_gain, opt_key, opt_moves, misc, misc0;
    uint32_t cur_len_max = 0;                 // longest read (cells) of the S1 call in flight
    uint64_t upload_epoch = 0, ord_epoch = ~0ull, ord_sig = 0;      // the cell orders in arith_ord belong to this set of contigs (signature) as uploaded then (epoch): S2 after S1, or the next step over a resident batch, reuses them
    const uint2* cur_ord = nullptr; const uint64_t* cur_ord_off = nullptr;      // ... of the S1 call in flight
    DevBuf arith_ord, arith_scr, arith_tab, arith_pool;      // reference-arithmetic mode: cell orders of the call's contigs, the order kernel's tables, prefix arrays, optimise scratch
    floria_timing timing{};
    // device-resident copy of the last S1 batch (floria_hip_hap_graph)
    uint64_t batch_token = 0, token_counter = 0;
    fl::BlockSet last_bs{};
    const uint8_t* last_part = nullptr;
    const uint32_t* last_best = nullptr;
    uint32_t last_nall = 2;
    std::vector<uint32_t> last_bc, last_start, last_end;
    std::vector<const floria_hip_contig*> last_contigs;      // the handles that batch was phased from (floria_hip_join_paths refuses any other array)
    DevBuf graph_buf, graph_hist, graph_sort;
    // uploads
    DevBuf up_tmp;                            // raw allele / qual bytes + the flatten kernel's tables (transient per upload)
    std::vector<Arena*> arena_cache;          // released batch arenas, reused by the next upload
    StagePool stage;                          // pinned staging ring for pageable sources
    DevBuf pile_in, pile_out;                 // floria_hip_pileup_records: blob + record arrays + SNP table + offsets, and the cell arrays
    // the cells of the last floria_hip_pileup_records_resident call, still in pile_in / pile_out (floria_hip_assemble_contigs); res_token 0 = none
    uint64_t res_token = 0;
    const floria_record_summary* res_summary = nullptr;
    uint32_t res_n_contigs = 0;
    std::vector<uint32_t> res_contig;         // contig of every record (header-sized; the plan is validated against it)
    const uint64_t* res_cell_off = nullptr; const uint32_t* res_snp = nullptr; const uint8_t *res_allele = nullptr, *res_qual = nullptr;
    const uint32_t* res_seq_pos = nullptr;    // ... and the walked sequence positions next to them (floria_hip_assemble_contigs_opt, KEEP_SEQ_POS)
    DevBuf asm_plan;                          // floria_hip_assemble_contigs: the fragment plan and the per-fragment cell counts / offsets
    DevBuf asm_ord_scr;                       // floria_hip_assemble_contigs_ordered: the general kernel's tables
    double mono_ms[6] = {};                   // the last floria_hip_drop_monomorphic call's device time by kind (floria_hip_mono_timing)
    DevBuf mono_buf;                          // floria_hip_drop_monomorphic: the per-SNP tables, the per-read survivor words and the call's small tables
    DevBuf span_buf;                          // floria_hip_read_spans: the groups, the contig table and the two result arrays (a buffer of its own: no residency ends)
    DevBuf hs_tmp;                            // floria_hip_reassign_batch_resident: the slot tables between its kernels (the handle has a buffer of its own); floria_hip_join_paths: its path tables
    DevBuf join_bits;                         // floria_hip_join_paths: the paths' bitmaps
    DevBuf inf_in;                            // floria_hip_inflate_bgzf: the compressed bytes and the per-member tables (the blob has a buffer of its own)
    DevBuf rec_in, rec_out, rec_names;        // floria_hip_blob_records: the chains' tables, the per-record arrays, the compacted names (buffers of their own: no residency ends)
    DevBuf seq_in, seq_out;                   // floria_hip_blob_sequences: the records' offsets, and the bases and qualities (buffers of their own: no residency ends)
    DevBuf est_in, est_win, est_cols;         // floria_hip_blob_estimate: the record arrays, one position window's arrays, one window's sampled columns (buffers of their own: no residency ends)
    uint32_t estimate_window = 0;             // (tests) floria_hip_blob_estimate: positions per window, 0 = 2^22
    uint32_t inflate_slots = 0;               // (tests) floria_hip_inflate_bgzf: members in flight, 0 = two per CU
    uint32_t stage_threads = 8;
};

// A batch of contigs uploaded together shares ONE device allocation (an arena): raw CSR regions filled by DMA, flattened
// regions written by flatten_kernel.  The arena is released when its last contig handle is freed (and then kept in a small
// per-context cache, so a host that uploads batch after batch never reallocates).
struct Arena {
    floria_hip_ctx* ctx = nullptr;
    DevBuf buf;
    uint32_t n_contigs = 0, refs = 0;
    uint64_t R = 0, C = 0;                                   // reads / cells of the batch
    size_t off_ro = 0, off_first = 0, off_last = 0;          // region offsets (bytes)
    std::vector<uint64_t> read_prefix;                       // [n_contigs+1]
    // host copies of first/last (haplogroup bookkeeping of S2 / get_hapq), fetched from the device on first use
    bool host_meta = false;
    std::vector<uint32_t> h_first, h_last;
};

struct floria_hip_contig {
    floria_hip_ctx* ctx = nullptr;
    Arena* arena = nullptr;
    uint32_t idx = 0;           // position inside the arena's batch
    uint32_t n_reads = 0;
    uint64_t n_cells = 0;
    uint32_t max_len = 0;       // max cells per read
    uint32_t n_alleles = 2;     // 2 or 4 (kernel template)
    bool has_q0 = false;        // some cell has qual 0 (weight 0): presence != (weight sum > 0)
    const uint32_t *h_first = nullptr, *h_last = nullptr;   // valid after host_meta(c)
    fl::ContigDev dev{};
    const uint32_t* seq_pos = nullptr;      // [n_cells] the SEQ_POS words (include/floria_hip.h) of a contig that carries positions, else null
};

namespace {

int ensure_binom(floria_hip_ctx* ctx, double eps, uint32_t nmax) {
    nmax = std::min(nmax, BINOM_NMAX_CAP);
    if (ctx->binom_eps == eps && ctx->binom_nmax >= nmax && ctx->d_binom.p) return 0;
    nmax = std::max(nmax, ctx->binom_eps == eps ? ctx->binom_nmax : 0u);
    std::vector<double> tab((size_t)(nmax + 1) * (nmax + 2) / 2);
    for (uint64_t n = 0; n <= nmax; ++n)
        for (uint64_t k = 0; k <= n; ++k) {
            // stable_binom_cdf_p_rev (utils_frags.rs:211-248), host libm
            double v = 0.0;
            if (n != 0) {
                double n64 = (double)n, k64 = (double)k;
                double a = k64 / n64;
                if (a == 1.0) a = 0.9999999;
                if (a == 0.0) a = 0.0000001;
                double rel_ent = a * std::log(a / eps) + (1.0 - a) * std::log((1.0 - a) / (1.0 - eps));
                if (a < eps) rel_ent = -rel_ent;
                v = -1.0 * n64 / DIV_FACTOR * rel_ent;
            }
            tab[n * (n + 1) / 2 + k] = v;
        }
    int rc = ctx->d_binom.ensure(tab.size() * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_binom.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->binom_eps = eps; ctx->binom_nmax = nmax;
    return 0;
}

int ensure_hash(floria_hip_ctx* ctx, uint32_t len) {
    if (ctx->hash_len >= len && ctx->d_hash.p) return 0;
    len = std::max<uint32_t>(len, 4 * fl::HASH_M);
    std::vector<uint64_t> t((size_t)len * 4);
    uint64_t s = 0x1577f10a1aull;
    for (uint32_t i = 0; i < len; ++i) {
        t[i] = splitmix64(s) | 1ull;                 // Rq1 (odd)
        t[(size_t)len + i] = splitmix64(s);          // Rp1
        t[(size_t)2 * len + i] = splitmix64(s) | 1ull;
        t[(size_t)3 * len + i] = splitmix64(s);
    }
    int rc = ctx->d_hash.ensure(t.size() * 8);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_hash.p, t.data(), t.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->hash_len = len;
    return 0;
}

struct EventTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    std::vector<int> kind;
    hipStream_t s;
    explicit EventTimer(hipStream_t st) : s(st) {}
    ~EventTimer() { for (auto& e : ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); } }
    std::vector<hipStream_t> on;
    int begin(int k, hipStream_t st = nullptr) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
        ev.push_back({a, b}); kind.push_back(k); on.push_back(st ? st : s);
        (void)hipEventRecord(a, on.back());
        return (int)ev.size() - 1;
    }
    void end(int i) { if (i >= 0) (void)hipEventRecord(ev[i].second, on[i]); }
    double elapsed(int i) { float ms = 0; if (i >= 0 && hipEventElapsedTime(&ms, ev[i].first, ev[i].second) == hipSuccess) return ms; return 0; }
    double sum(int k) {
        double t = 0;
        for (size_t i = 0; i < ev.size(); ++i) if (kind[i] == k) { float ms = 0; if (hipEventElapsedTime(&ms, ev[i].first, ev[i].second) == hipSuccess) t += ms; }
        return t;
    }
    // wall time during which at least one launch of kind k was in flight (the launches of the job groups overlap on separate streams: their durations add up to
    // more than the wall clock, this does not)
    double union_ms(int k) {
        std::vector<std::pair<float, float>> iv;
        for (size_t i = 0; i < ev.size(); ++i) if (kind[i] == k) {
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, ev.front().first, ev[i].first) == hipSuccess && hipEventElapsedTime(&b, ev.front().first, ev[i].second) == hipSuccess) iv.push_back({a, b});
        }
        std::sort(iv.begin(), iv.end());
        double t = 0; float lo = 0, hi = -1;
        for (auto& x : iv) { if (hi < lo || x.first > hi) { if (hi >= lo) t += hi - lo; lo = x.first; hi = x.second; } else if (x.second > hi) hi = x.second; }
        if (hi >= lo) t += hi - lo;
        return t;
    }
    double span() {
        if (ev.empty()) return 0;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.front().first, ev.back().second);
        return ms;
    }
    void publish(floria_timing& tm);
};
enum { K_BEAM = 0, K_OPT = 1, K_SEL = 2, K_H2D = 3, K_D2H = 4, K_REASSIGN = 5, K_PHASE = 6, K_PILEUP = 7 };
// the closing line of every call but S1 (which has fields and rules of its own): the sums by kind and the span, into a timing the call reset when it began
// (a kind the call never timed sums to the 0 the field holds anyway)
void EventTimer::publish(floria_timing& tm) {
    tm.h2d_ms = sum(K_H2D); tm.d2h_ms = sum(K_D2H); tm.pileup_ms = sum(K_PILEUP); tm.select_ms = sum(K_SEL); tm.reassign_ms = sum(K_REASSIGN); tm.total_ms = span();
}

void sync_all(floria_hip_ctx* ctx) {
    for (uint32_t g = 0; g < floria_hip_ctx::MAX_LANES; ++g) if (ctx->gstream[g]) (void)hipStreamSynchronize(ctx->gstream[g]);
    for (uint32_t g = 0; g < floria_hip_ctx::MAX_LANES; ++g) if (ctx->gstream_low[g]) (void)hipStreamSynchronize(ctx->gstream_low[g]);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->flat_stream) (void)hipStreamSynchronize(ctx->flat_stream);
    (void)hipStreamSynchronize(ctx->stream);
}

// ---- S1 launch plan ---------------------------------------------------------------------------------------------------------
// The per-ploidy loop of get_local_hap_blocks (graph_processing.rs:132-252) runs as STAGES: a stage is a set of consecutive
// ploidies whose (beam -> optimise) chains run concurrently, each on its own stream with its own scratch slice ("lane"), followed
// by the stop rule (select_kernel) for the stage's ploidies in ascending order.  The default is one ploidy per stage (no
// speculative work: the launches of ploidy p+1 skip the blocks whose stop rule fired at p).  A ploidy run never reads an earlier
// ploidy's result (only the stop rule does, :198-251), so running several ploidies of a block at once gives identical results;
// it trades extra (block, ploidy) jobs for a shorter dependent chain and is used when the batch cannot fill the chip.
// JOB GROUPS: the non-empty blocks are dealt into G groups whose stage sequences run independently on separate streams, so one
// group's launch tail (persistent waves draining their last jobs) is filled by the other group's kernels.
// A lane (group g, position j inside the stage) owns the SAME byte slice of every scratch pool for the whole call — sized for
// the largest ploidy — so kernels of different groups/ploidies that are live at the same time can never alias.
// threshold of the MEC-ratio stop rule for ploidy p (graph_processing.rs:204-220), libm pow as in the reference
double mec_threshold(const floria_params* prm, uint32_t p) {
    const double eps = prm->epsilon, pl = (double)p;
    if (prm->ploidy_sensitivity == 1) return 1.0 / (1.0 - eps) / (1.0 + 1.0 / (std::pow(pl, 0.50) + 1.00));
    if (prm->ploidy_sensitivity == 2) return 1.0 / (1.0 - eps) / (1.0 + 1.0 / (std::pow(pl, 1.00) + 1. / 3.));
    return 1.0 / (1.0 - eps) / (1.0 + 1.0 / (std::pow(pl, 1.00) + 1.00));
}

struct PloidyPlan {
    uint32_t p = 0, LM = 0;
    bool shortcut = false, wide = false, slab = false, beam_spec = false;
    uint64_t state_bytes = 0, hist_stride = 0;
    fl::SlabLds SL{}; fl::WideLds WL{}; fl::BeamLds LY{};
    uint32_t beam_slots = 0;
    uint64_t cand_cap = 1;
    uint32_t threads = 128, opt_slots = 0;
    size_t opt_lds = 0;
    bool hl = false, opt_spec = false;
    bool opt_pk = false;          // optimise: the packed-cell instances (their weight table shares LDS with the candidate sort: no bytes of its own)
    uint32_t pm_lds_off = 0;      // optimise: where the visiting order of the reads (u16, longest first) sits in the workgroup's LDS (0 = none: the reads in block order)
    uint32_t fk_lds_off = 0;      // ... and the first-insertion keys as 32-bit words
    uint32_t fx_tags = 0;         // ... and the words of a map's claim table
    uint32_t fx_lds_off = 0;      // reference-arithmetic mode: where the emulated position maps sit in the workgroup's LDS (0 = in HBM scratch)
};

// the blocks of an S1 call as the launch plan sees them
struct PhaseShape {
    fl::BlockSet bs{};
    bool any_q0 = false;                // some cell has qual 0
    uint32_t n_jobs = 0;                // non-empty blocks
    uint64_t tot_reads = 0;             // reads of all blocks
    uint32_t n_max = 1, span_max = 1;   // most reads / widest SNP span of one block
    bool all_pk = false;                // every contig with reads carries packed cells (ContigDev::cell_pk)
};

// s1_core's per-call device arrays that the launch loop reads and writes
struct PhaseBufs {
    const uint32_t* jobs;                                   // the non-empty blocks, group after group
    uint8_t* planes;                                        // every read's partition, one plane per ploidy
    uint8_t* beam_part;                                     // beam partitions, one plane per position in a stage (+1: the tail launch's, below)
    double* mec; double* na; uint32_t* iters;               // per (block, ploidy)
    uint8_t* done; uint32_t* best; uint32_t* tried;         // per block: the stop rule's state ...
    uint32_t* stop; uint32_t* ready;                        // ... and what speculative stages publish of it
    uint32_t* queue;                                        // persistent-grid queue heads: a pair per (lane, ploidy)
    double* margin; uint32_t* diag; unsigned long long* steps;
};

// ---- runtime selector -> compile-time constant, for the two launchers below ---------------------------------------------------
template <class F> auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// f(V) for the first V that equals v, the last V otherwise (the plan guarantees one of them)
template <int V, int... Vs, class F> auto pick(uint32_t v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else return v == (uint32_t)V ? f(std::integral_constant<int, V>{}) : pick<Vs...>(v, f);
}

// The one place where a ploidy's plan becomes a beam-search kernel instance:
//   beam_slab_kernel<A, Q0, 0, 0, SPEC, ARITH>, and <2, false, p = 2..5, 10, SPEC, ARITH> where the plan says beam_spec (biallelic, no q = 0 cell, beam 10);
//   beam_wide_kernel<A, Q0, ARITH>; beam_kernel<A, ARITH> (the generic kernel).
// spec: the launch may drop jobs (a speculative stage, or the tail launch that waits for the stop rule): only the SPEC instances carry those checks.
template <int A>
hipError_t launch_beam(const PloidyPlan& q, bool arith, bool any_q0, bool spec, uint32_t slots, hipStream_t st, const fl::BeamArgs& a) {
    auto go = [&](auto kern, uint32_t lds, bool big_lds) -> hipError_t {      // (the wide and the generic kernel may ask for more than 48 KB of LDS)
        if (big_lds && lds > 48 * 1024) { const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(kern, dim3(slots), dim3(64), lds, st, a);
        return hipGetLastError();
    };
    return with_bool(arith, [&](auto AR) {
        if (q.slab) return with_bool(spec, [&](auto SP) {
            if (q.beam_spec) return pick<2, 3, 4, 5>(q.p, [&](auto TP) { return go(fl::beam_slab_kernel<2, false, TP, 10, SP, AR>, q.SL.total, false); });
            return with_bool(any_q0, [&](auto Q0) { return go(fl::beam_slab_kernel<A, Q0, 0, 0, SP, AR>, q.SL.total, false); });
        });
        if (q.wide) return with_bool(any_q0, [&](auto Q0) { return go(fl::beam_wide_kernel<A, Q0, AR>, q.WL.total, true); });
        return go(fl::beam_kernel<A, AR>, q.LY.total, true);
    });
}

// The one place where a ploidy's plan becomes an optimise kernel instance:
//   optimize_kernel<A, HL, THREADS = 128 | 512 | 1024>, and <2, true, 512 | 1024, p = 1..5> where the plan says opt_spec, <2, true, 512, p = 1..5, false, 0, PK = true> where it also
//   says opt_pk (packed cells);
//   reference arithmetic: <A, HL, THREADS, 0, true>, <A, true, 512, 0, true, 4>, and <2, true, 512, p = 1..5, true, 0 | 4> (biallelic, histogram in LDS, ploidy <= 5).
template <int A>
hipError_t launch_optimize(const PloidyPlan& q, const Knobs& K, uint32_t slots, hipStream_t st, const fl::OptArgs& a) {
    auto go = [&](auto kern) -> hipError_t {
        if (q.opt_lds > 48 * 1024) { const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.opt_lds); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(kern, dim3(slots), dim3(q.threads), q.opt_lds, st, a);
        return hipGetLastError();
    };
    if (K.arith) {
        // (LDS allows two workgroups per CU: four waves per SIMD, 128 VGPRs)
        const bool two_wg = q.hl && q.threads == 512 && std::min<size_t>((156 * 1024) / (q.opt_lds + 8 * 1024), 2048 / q.threads) <= 2 && !K.arith_ow6;
        // reference arithmetic, 512 threads, histogram in LDS, biallelic, ploidy <= 5 (every BASELINE config at the CLI's defaults): ploidy-specialised instances
        // (round 6: the per-partition loops unroll, `pair / p` is a multiplication); four waves per SIMD (128 VGPRs) where LDS allows two workgroups per CU anyway
        if (q.hl && q.threads == 512 && A == 2 && q.p <= 5 && !K.no_specialized)
            return with_bool(two_wg, [&](auto TW) { return pick<1, 2, 3, 4, 5>(q.p, [&](auto TP) { return go(fl::optimize_kernel<2, true, 512, TP, true, TW ? 4 : 0>); }); });
        if (two_wg) return go(fl::optimize_kernel<A, true, 512, 0, true, 4>);
        return with_bool(q.hl, [&](auto HL) { return pick<1024, 512, 128>(q.threads, [&](auto T) { return go(fl::optimize_kernel<A, HL, T, 0, true>); }); });
    }
    if (q.opt_spec && q.opt_pk) return pick<1, 2, 3, 4, 5>(q.p, [&](auto TP) { return go(fl::optimize_kernel<2, true, 512, TP, false, 0, true>); });
    if (q.opt_spec) return pick<1024, 512>(q.threads, [&](auto T) { return pick<1, 2, 3, 4, 5>(q.p, [&](auto TP) { return go(fl::optimize_kernel<2, true, T, TP>); }); });
    return with_bool(q.hl, [&](auto HL) { return pick<1024, 512, 128>(q.threads, [&](auto T) { return go(fl::optimize_kernel<A, HL, T>); }); });
}

// ---- plan every ploidy once: kernel choice, grid, scratch per slot (host only) ---------------------------------------------------
template <int A>
int plan_ploidies(const floria_hip_ctx* ctx, const floria_params* prm, const PhaseShape& S, uint32_t nj_max, std::vector<PloidyPlan>& plan) {
    const uint32_t P = prm->max_ploidy, B = prm->beam;
    const Knobs& K = ctx->knobs;
    const bool any_q0 = S.any_q0;
    const uint32_t n_max = S.n_max, span_max = S.span_max;
    plan.assign(P + 1, PloidyPlan{});
    const uint64_t fx_ctrl = fl::fx_ctrl_bytes(span_max + 1);       // (+1: slack)
    const uint32_t mean_n = (uint32_t)(S.tot_reads / std::max<uint32_t>(1, S.n_jobs));
    for (uint32_t p = 1; p <= P; ++p) {
        PloidyPlan& q = plan[p];
        q.p = p; q.LM = p * B;
        const uint32_t LM = q.LM;
        if (LM > 65000) return fail(FLORIA_E_UNSUPPORTED, "ploidy*beam too large");
        // ploidy 1 has nothing to search: one state, one partition, every child passes (p_k - lse == 0 > ln 0.01), the
        // partition is "all reads in haplotype 0" (global_clustering.rs:74-134 with ploidy == 1) -> a memset.
        q.shortcut = p == 1 && !K.no_p1_shortcut;
        q.state_bytes = (uint64_t)LM * span_max * p * A * 8;
        // traceback records + the slab kernels' per-slab tables that live in HBM (window-exit hash terms; everything for wide beams)
        q.hist_stride = (((uint64_t)fl::beam_hist_off(n_max, LM, B) + LM + 64 + 1) & ~1ull) + fl::SLAB_DUMMY_WORDS + std::max<uint64_t>(4ull * LM * p, fl::wide_scratch_words(LM, p, any_q0, K.arith != 0));   // + the dummy words of beam_slab_kernel's branch-free tails
        const bool arith_slab = K.arith && K.beam_path != 1;      // the reference's running sums on the shared slabs (beam_slab_kernel<.., ARITH = true>)
        q.SL = fl::slab_lds_layout(LM, p, any_q0, arith_slab);
        q.WL = fl::wide_lds_layout(LM, p, any_q0);
        q.LY = fl::beam_lds_layout(LM);
        q.beam_spec = A == 2 && !any_q0 && B == 10 && p >= 2 && p <= 5 && !K.no_specialized;
        const uint32_t by_lds = std::max<uint32_t>(1, (uint32_t)((158 * 1024) / (q.SL.total + 256)));
        const uint32_t waves_per_simd = (uint32_t)fl::slab_waves(q.beam_spec ? (int)p : 0);
        q.beam_slots = ctx->user_slots ? ctx->user_slots : (uint32_t)ctx->n_cu * std::min<uint32_t>(4 * waves_per_simd, by_lds);
        q.beam_slots = std::min(q.beam_slots, nj_max);
        const uint64_t slab_code_bytes = (uint64_t)LM * p * ((span_max + 15u) & ~15u);              // beam_slab_kernel: one code byte per (slab, position)
        const bool fits32 = q.state_bytes + slab_code_bytes < 0xf0000000ull;
        // shared-slab kernels: register heap for ploidy*beam <= 63 (the CLI defaults give <= 50), LDS heap beyond; the generic kernel
        // (per-state slabs, any size) remains for beams whose slab tables fit neither
        const bool wide_ok = fits32 && LM * p <= (uint32_t)fl::WIDE_NS_MAX && LM < 65000 && q.WL.total <= 150 * 1024;
        // (narrow sums: the register-heap slab kernel keeps biallelic sums in 40 bits, beam_slab_kernel.h; a block of >= 65 536 reads goes down the wide / generic kernels)
        const bool narrow = A == 2 && !any_q0;
        q.slab = LM <= 63 && fits32 && LM * p <= (uint32_t)fl::SLAB_NS_MAX && q.SL.total <= 60 * 1024 && !(narrow && n_max >= 65536u);
        q.wide = !q.slab && wide_ok;
        switch (K.beam_path) {                               // dev/test knob
            case 1: q.wide = false; q.slab = false; break;                     // generic
            case 2: q.wide = false; break;                                     // slab (where it applies, else generic)
            case 3: q.wide = wide_ok; q.slab = q.slab && !wide_ok; break;      // wide (where it applies)
            default: break;
        }
        if (K.arith && q.slab && arith_slab) {               // the reference's running sums on the shared slabs: LDS (the terms of a step) allows two waves per SIMD
            q.wide = false;
            q.beam_slots = std::min<uint32_t>(nj_max, ctx->user_slots ? ctx->user_slots : (uint32_t)ctx->n_cu * std::min<uint32_t>(4 * fl::SLAB_WAVES_ARITH, by_lds));
        } else if (K.arith && q.wide && K.beam_path != 1) {  // ... on the shared slabs of a wide beam (beam_wide_kernel<.., ARITH = true>: one lane per live slab walks the cells)
            q.slab = false; q.beam_spec = false;
        } else if (K.arith) {                                // ... or the generic kernel, whose lanes walk a read's cells one by one (beams whose slab tables fit neither shared-slab kernel)
            q.slab = false; q.wide = false; q.beam_spec = false;
            q.LY = fl::beam_lds_layout(LM, p);
            q.beam_slots = std::min<uint32_t>(nj_max, ctx->user_slots ? ctx->user_slots : (uint32_t)ctx->n_cu * std::min<uint32_t>(16, std::max<uint32_t>(1, (uint32_t)((158 * 1024) / (q.LY.total + 256)))));
        }
        // (narrow sums: low words, high bytes and code bytes over one position-index space of NS * span_pad + SLAB_PAD_IDX entries, beam_slab_kernel.h)
        const uint64_t narrow_bytes = (((uint64_t)LM * p * ((span_max + 15u) & ~15u) + fl::SLAB_PAD_IDX) * 11ull + 255ull) & ~255ull;
        if (q.slab && narrow && narrow_bytes >= 0xf0000000ull) q.slab = false;
        if (q.slab) q.state_bytes = narrow ? narrow_bytes : q.state_bytes + slab_code_bytes;
        if (!q.shortcut) {
            if (q.LY.total > 160 * 1024 - 64) return fail(FLORIA_E_UNSUPPORTED, "ploidy*beam needs more LDS than a CU has");
            if (q.wide) q.beam_slots = std::min<uint32_t>(q.beam_slots, (uint32_t)ctx->n_cu * std::max<uint32_t>(1, (uint32_t)((158 * 1024) / (q.WL.total + 512))));
        }
        // optimise
        while (q.cand_cap < (uint64_t)n_max * std::max(1u, p - 1)) q.cand_cap <<= 1;
        uint32_t threads = mean_n >= 384 ? 1024 : (mean_n >= 96 ? 512 : 128);
        if (K.opt_threads == 1024 || K.opt_threads == 512 || K.opt_threads == 128) threads = K.opt_threads;
        const size_t moved_bytes = ((((size_t)n_max + 31) / 32) * 4 + 15) & ~(size_t)15;
        const size_t hist_bytes = (size_t)span_max * p * A * 8;
        const size_t meta_bytes = n_max <= (uint32_t)fl::OPT_META_MAX ? (((size_t)n_max * 12 + 15) & ~(size_t)15) : 0;
        q.hl = hist_bytes + (size_t)span_max * p + 32 + moved_bytes + meta_bytes <= 60 * 1024 && !K.opt_global;
        const size_t code_bytes = q.hl ? ((size_t)span_max * p + 15) & ~(size_t)15 : 0;       // one byte per (position, partition), see optimize_kernel.h
        q.opt_lds = moved_bytes + meta_bytes + (q.hl ? ((hist_bytes + 15) & ~(size_t)15) + code_bytes : 0);
        // where the ploidy-specialised instances apply (75-92 VGPRs), three 512-thread workgroups per CU beat one of 1024 threads
        if (A == 2 && q.hl && p <= 5 && threads == 1024 && !K.opt_threads && !K.no_specialized) threads = 512;
        q.threads = threads;
        q.opt_spec = A == 2 && q.hl && threads >= 512 && p <= 5 && !K.no_specialized && !K.arith;
        auto wg_per_cu = [&](size_t lds) { return std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((156 * 1024) / (lds + 8 * 1024)), 2048 / threads)); };
        if (K.arith && !K.arith_hbm) {
            // the emulated position maps: control bytes (which every probe reads) + the claim words of a batched insertion, and the first-insertion keys as 32-bit words, in
            // LDS where that still leaves two workgroups per CU; the claim table as large as costs no workgroup (a table of fewer words than buckets makes false conflicts)
            const size_t cap = 68 * 1024;
            auto fx_sz = [&](uint32_t tags) { return (size_t)p * (2 * fx_ctrl + 4 * tags); };
            const size_t fk_sz = ((size_t)p * span_max * 4 + 15) & ~(size_t)15;
            const bool fk_ok = n_max < (1u << 20) && ctx->cur_len_max < 4096u;
            uint32_t tags = fl::FX_TAGS_MIN;
            if (q.opt_lds + fx_sz(tags) + 16 <= cap) {
                const bool fk = fk_ok && q.opt_lds + fx_sz(tags) + fk_sz + 16 <= cap;
                const size_t rest = q.opt_lds + (fk ? fk_sz : 0) + 16;
                const uint32_t tmax = std::min<uint32_t>(fl::FX_TAGS_MAX, K.fx_tags ? K.fx_tags : fl::fx_buckets_for(span_max + 1));
                while (tags * 2 <= tmax && rest + fx_sz(tags * 2) <= cap && wg_per_cu(rest + fx_sz(tags * 2)) == wg_per_cu(rest + fx_sz(fl::FX_TAGS_MIN))) tags *= 2;
                q.fx_lds_off = (uint32_t)q.opt_lds; q.opt_lds += fx_sz(tags); q.fx_tags = tags;
                if (fk) { q.fk_lds_off = (uint32_t)q.opt_lds; q.opt_lds += fk_sz; }
            } else if (fk_ok && q.opt_lds + fk_sz + 16 <= cap) { q.fk_lds_off = (uint32_t)q.opt_lds; q.opt_lds += fk_sz; }
        }
        q.opt_lds += 16;
        {   // the visiting order of the build / distance passes (optimize_kernel.h: u16 per read), where it costs no workgroup per CU
            const size_t pm_bytes = (((size_t)n_max * 2) + 15) & ~(size_t)15;
            if (!K.arith && !K.opt_block_order && meta_bytes && n_max <= 65535u && q.opt_lds + pm_bytes <= 60 * 1024 && wg_per_cu(q.opt_lds + pm_bytes) == wg_per_cu(q.opt_lds)) {
                q.pm_lds_off = (uint32_t)q.opt_lds; q.opt_lds += pm_bytes;
            }
        }
        // the packed-cell instances (optimize_kernel<.., PK = true>: biallelic, histogram in LDS, ploidy <= 5, 512 threads); their weight table takes no LDS of its own
        q.opt_pk = K.opt_packed && S.all_pk && q.opt_spec && threads == 512;
        uint32_t per_cu = wg_per_cu(q.opt_lds);
        per_cu = std::min<uint32_t>(per_cu, 8);
        q.opt_slots = std::min<uint32_t>((uint32_t)ctx->n_cu * per_cu, nj_max);
    }
    return 0;
}

// ---- scratch: one fixed slice per lane, sized for the largest ploidy -------------------------------------------------------------
struct LaneScratch { uint64_t state = 0, hist = 0, ohist = 0, odist = 0, ogain = 0, okey = 0, omoves = 0, arith = 0; };      // bytes of a lane's slice of each pool
uint64_t sort_cap_of(uint32_t p, uint32_t span_max) { uint64_t c = 1; while (c < (uint64_t)p * span_max) c <<= 1; return c; }

template <int A>
int size_scratch(floria_hip_ctx* ctx, const PhaseShape& S, uint32_t n_lanes, std::vector<PloidyPlan>& plan, LaneScratch& sl) {
    const uint32_t P = (uint32_t)plan.size() - 1, n_max = S.n_max, span_max = S.span_max;
    const uint64_t fx_bytes = fl::fx_ctrl_bytes(span_max + 1) + fl::fx_slot_bytes(span_max + 1);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = (uint64_t)((double)(free_b + ctx->state_pool.cap + ctx->hist_pool.cap) * 0.6);
    for (;;) {
        uint64_t need = 0;
        for (uint32_t p = 1; p <= P; ++p) if (!plan[p].shortcut) need = std::max(need, (plan[p].state_bytes + plan[p].hist_stride * 4) * plan[p].beam_slots);
        if (need * n_lanes <= budget) break;
        bool shrunk = false;
        for (uint32_t p = 1; p <= P; ++p) if (!plan[p].shortcut && (plan[p].state_bytes + plan[p].hist_stride * 4) * plan[p].beam_slots == need && plan[p].beam_slots > 1) { plan[p].beam_slots /= 2; shrunk = true; }
        if (!shrunk) break;
    }
    auto up256 = [](uint64_t x) -> uint64_t { return (x + 255) & ~(uint64_t)255; };
    sl = LaneScratch{};
    for (uint32_t p = 1; p <= P; ++p) {
        const PloidyPlan& q = plan[p];
        if (!q.shortcut) { sl.state = std::max(sl.state, up256(q.state_bytes * q.beam_slots)); sl.hist = std::max(sl.hist, up256(q.hist_stride * 4 * q.beam_slots)); }
        sl.ohist = std::max(sl.ohist, up256((uint64_t)q.opt_slots * span_max * p * A * 8));
        sl.odist = std::max(sl.odist, up256((uint64_t)q.opt_slots * n_max * p * 8));
        sl.ogain = std::max(sl.ogain, up256((uint64_t)q.opt_slots * q.cand_cap * 8));
        sl.okey = std::max(sl.okey, up256((uint64_t)q.opt_slots * q.cand_cap * 4));
        sl.omoves = std::max(sl.omoves, up256((uint64_t)q.opt_slots * n_max * 4));
        if (ctx->knobs.arith) sl.arith = std::max(sl.arith, up256((uint64_t)q.opt_slots * ((uint64_t)p * span_max * 8 + sort_cap_of(p, span_max) * 12 + (uint64_t)p * 2 * fx_bytes + 16 + (uint64_t)p * span_max * 8) + 64));
    }
    // (a pool that has to grow is freed first: hipFree synchronises the device, and nothing of this call is in flight yet)
    int rc = ctx->state_pool.ensure(sl.state * n_lanes); if (rc) return rc;
    rc = ctx->hist_pool.ensure(sl.hist * n_lanes); if (rc) return rc;
    rc = ctx->opt_hist.ensure(sl.ohist * n_lanes); if (rc) return rc;
    rc = ctx->opt_dist.ensure(sl.odist * n_lanes); if (rc) return rc;
    rc = ctx->opt_gain.ensure(sl.ogain * n_lanes); if (rc) return rc;
    rc = ctx->opt_key.ensure(sl.okey * n_lanes); if (rc) return rc;
    rc = ctx->opt_moves.ensure(sl.omoves * n_lanes); if (rc) return rc;
    if (ctx->knobs.arith) { rc = ctx->arith_pool.ensure(sl.arith * n_lanes); if (rc) return rc; }
    return 0;
}

// ---- streams and events: lane (g, j) runs on its own stream; lane (0, 0) is the context's main stream -----------------------------
int lane_streams(floria_hip_ctx* ctx, uint32_t n_lanes, uint32_t W, bool spec_first, hipStream_t* ls) {
    for (uint32_t l = 0; l < n_lanes; ++l) {
        if (l == 0) { ls[0] = ctx->stream; continue; }
        if (W > 1 && (l % W) >= (spec_first ? 3u : 1u)) {      // ({1}{2}{3}{4..P}: the lanes of ploidy >= 5)        // a speculative stage's lanes of ploidy >= 4: lowest dispatch priority, so that the ploidies every
                                                                // block needs get the wave slots first and the stop rule is known before most of these jobs start
            if (!ctx->gstream_low[l]) {
                int least = 0, greatest = 0;
                (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
                if (hipStreamCreateWithPriority(&ctx->gstream_low[l], hipStreamNonBlocking, least) != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipStreamCreateWithFlags(&ctx->gstream_low[l], hipStreamNonBlocking)); }
            }
            if (!ctx->ev_join[l]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_join[l], hipEventDisableTiming));
            if (!ctx->ev_fork[l]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork[l], hipEventDisableTiming));
            ls[l] = ctx->gstream_low[l];
            continue;
        }
        if (!ctx->gstream[l]) HIPCHK(hipStreamCreateWithFlags(&ctx->gstream[l], hipStreamNonBlocking));
        if (!ctx->ev_join[l]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_join[l], hipEventDisableTiming));
        if (!ctx->ev_fork[l]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork[l], hipEventDisableTiming));
        ls[l] = ctx->gstream[l];
    }
    if (!ctx->ev_fork[0]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork[0], hipEventDisableTiming));
    return 0;
}

// ---- the stage loop: every group's stages, each a beam -> optimise chain per ploidy, then the stop rule ---------------------------
template <int A>
int run_phase(floria_hip_ctx* ctx, const floria_params* prm, const PhaseShape& S, const std::vector<uint32_t>& group_off, const std::vector<std::vector<uint32_t>>& stages,
              hipEvent_t* chunk_ev, const PhaseBufs& D, EventTimer& T, bool& p1_shortcut) {
    const uint32_t P = prm->max_ploidy, B = prm->beam;
    const Knobs& K = ctx->knobs;
    p1_shortcut = false;
    const uint32_t G = (uint32_t)group_off.size() - 1;
    if (S.n_jobs == 0) return 0;
    const fl::BlockSet& bs = S.bs;
    const uint64_t tot_reads = S.tot_reads;
    const uint32_t n_max = S.n_max, span_max = S.span_max;
    uint32_t W = 1;                                        // widest stage
    for (auto& st : stages) W = std::max<uint32_t>(W, (uint32_t)st.size());
    const uint32_t n_lanes = G * W;
    if (n_lanes > floria_hip_ctx::MAX_LANES) return fail(FLORIA_E_INVALID, "internal: too many launch lanes");
    uint32_t nj_max = 0;
    for (uint32_t g = 0; g < G; ++g) nj_max = std::max(nj_max, group_off[g + 1] - group_off[g]);
    const double cutoff = std::log(PROB_CUTOFF);      // graph_processing.rs:146
    std::vector<PloidyPlan> plan;
    int rc = plan_ploidies<A>(ctx, prm, S, nj_max, plan); if (rc) return rc;
    LaneScratch sl;
    rc = size_scratch<A>(ctx, S, n_lanes, plan, sl); if (rc) return rc;
    hipStream_t ls[floria_hip_ctx::MAX_LANES];
    rc = lane_streams(ctx, n_lanes, W, stages.front().size() > 1, ls); if (rc) return rc;
    const uint64_t fx_ctrl = fl::fx_ctrl_bytes(span_max + 1), fx_slot = fl::fx_slot_bytes(span_max + 1), fx_bytes = fx_ctrl + fx_slot;       // (+1: slack)
    const int t_phase = T.begin(K_PHASE);
    // ploidy 1 (always position 0 of the first stage) without a search: its beam partition is all zeros, for every group's reads
    // ... or without a launch at all (ploidy_stages left its stage out): the ploidy-2 optimise job stands for it, and plane 0 of D.planes was zeroed with the call's memset
    const bool p1_fused = stages.front().front() == 2;
    if (p1_fused) p1_shortcut = true;
    else if (plan[1].shortcut) { HIPCHK(hipMemsetAsync(D.beam_part, 0, tot_reads, ctx->stream)); p1_shortcut = true; }
    // fork: every group's first lane starts after what the main stream has queued so far (uploads, memsets, block_reads_kernel)
    if (G > 1) {
        HIPCHK(hipEventRecord(ctx->ev_fork[0], ctx->stream));
        for (uint32_t g = 1; g < G; ++g) HIPCHK(hipStreamWaitEvent(ls[g * W], ctx->ev_fork[0], 0));
    }
    // chunked inputs: group g's first lane also waits until chunk g's cells have arrived and been flattened
    if (chunk_ev) for (uint32_t g = 0; g < G; ++g) HIPCHK(hipStreamWaitEvent(ls[g * W], chunk_ev[g], 0));
    const uint64_t* H = ctx->d_hash.as<uint64_t>();
    // Per-block dataflow for the tail of a one-ploidy-per-stage plan (graph_processing.rs:132-252 runs a block's ploidies back to back and stops): few blocks reach
    // the last ploidy, so its beam launch is a handful of lone-wave chains as long as the longest block — behind the optimise launch of the ploidy below, which the
    // same long blocks keep waiting.  With tail_p != 0 that beam launch is queued on a stream of its own right behind the beam launch of tail_p - 1: it runs BESIDE
    // the optimise launch, a small persistent grid whose jobs each wait for their block's stop rule (tried[b] >= tail_p - 1 or blk_done[b], beam_slab_kernel.h), in
    // the order the optimise launch works through them; it writes its partitions into a plane of its own.  Nothing waits for this launch but the last optimise launch.
    uint32_t tail_p = 0;
    {
        const bool want = K.tail_overlap > 0;      // (measured on config 4: no gain — the optimise launch it hides is 1.2-1.7 ms when the chip is otherwise idle, and the waiting grid costs as much: profiles/r04_tail_overlap_ab.txt)
        if (want && W == 1 && stages.size() >= 3 && P >= 3 && stages.back().size() == 1 && stages.back()[0] == P && stages[stages.size() - 2][0] == P - 1
            && plan[P].slab && !plan[P].wide && !plan[P].shortcut && !plan[P - 1].shortcut && !K.arith && ctx->hw_queues >= 5 && G <= floria_hip_ctx::MAX_GROUPS) tail_p = P;
    }
    uint8_t* const tail_part = D.beam_part + (uint64_t)W * (tot_reads + 16);
    // one beam launch of group g: ploidy p on stream st (scratch slice `lane`), partitions into lane_part.  wait_tried != 0: the launch of the last ploidy that runs
    // beside the optimise launch of ploidy wait_tried (per-block dataflow, below)
    auto beam_launch = [&](const std::vector<uint32_t>& stage, uint32_t g, uint32_t nj, const uint32_t* gjobs, uint32_t p, uint32_t lane, hipStream_t st, uint32_t* gqueue,
                           uint8_t* lane_part, uint32_t wait_tried) -> int {
        const PloidyPlan& q = plan[p];
        const uint32_t slots_full = std::min(q.beam_slots, nj);
        fl::BeamArgs a{};
        a.bs = bs; a.job_block = gjobs; a.n_jobs = nj; a.ploidy = p; a.beam = B; a.span_max = span_max; a.n_max = n_max;
        a.queue_head = gqueue; a.blk_done = D.done; a.stop_at = stage.size() > 1 && !wait_tried ? D.stop : nullptr;
        a.tried = D.tried; a.wait_tried = wait_tried; a.wait_ticks = 2000000u;      // (20 ms: longer than any optimise launch takes)
        a.state_pool = (uint64_t*)(ctx->state_pool.as<char>() + sl.state * lane); a.state_stride = q.state_bytes;
        a.hist_pool = (uint32_t*)(ctx->hist_pool.as<char>() + sl.hist * lane); a.hist_stride = q.hist_stride;
        a.binom_tab = ctx->d_binom.as<double>(); a.binom_nmax = ctx->binom_nmax;
        a.eps = prm->epsilon; a.div_factor = DIV_FACTOR; a.cutoff = cutoff;
        a.ln_eps = (float)std::log(prm->epsilon); a.ln_1meps = (float)std::log(1.0 - prm->epsilon);
        a.Rq1 = H; a.Rp1 = H + ctx->hash_len; a.Rq2 = H + 2ull * ctx->hash_len; a.Rp2 = H + 3ull * ctx->hash_len;
        a.part_out = lane_part; a.job_margin = D.margin; a.max_ploidy = P; a.diag = D.diag; a.steps_done = D.steps;
        a.prof = (unsigned long long*)(D.diag + 4);
        a.no_bulk = K.no_bulk;
        a.cell_ord = ctx->cur_ord; a.cell_ord_off = ctx->cur_ord_off;
        const bool gated = !wait_tried && stage.size() > 1 && ((stage[0] <= 2 && p >= 4) || (stage[0] == 4 && p >= 5));      // (ungated ploidy 4 / 5 measured worse: 24.3 against 22.5 ms for the 250-contig shard)
        // ... and with a smaller persistent grid: the optimise workgroups of the lower ploidies (whose results decide which of these
        // jobs are needed at all) find room on the chip, and jobs that are dequeued later are dropped more often
        const uint32_t slots = wait_tried ? std::max<uint32_t>(1, std::min(slots_full, (uint32_t)ctx->n_cu * K.tail_waves)) : gated ? std::max<uint32_t>(1, std::min(slots_full, std::max<uint32_t>((uint32_t)ctx->n_cu, slots_full / K.spec_gate_div))) : slots_full;
        if (gated) {          // ploidies few blocks need start when ploidy 2 has left the chip: by the time their jobs run, the stop rule of most
                              // blocks is known and the jobs are dropped at dequeue or within 64 reads
            if (!ctx->ev_gate[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_gate[g], hipEventDisableTiming));
            HIPCHK(hipStreamWaitEvent(st, ctx->ev_gate[g], 0));
        }
        const int t = T.begin(K_BEAM, st);
        HIPCHK(launch_beam<A>(q, K.arith != 0, S.any_q0, a.stop_at != nullptr || wait_tried != 0, slots, st, a));      // (a speculative stage or the tail launch: the instances that can drop a job)
        T.end(t);
        ctx->timing.beam_launches++;
        if (!wait_tried && stage.size() > 1 && ((stage[0] <= 2 && p == 2) || (stage[0] == 4 && p == 4))) {          // (the beam search of ploidy 2 opens the gate; ploidy 3 measured worse)
            if (!ctx->ev_gate[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_gate[g], hipEventDisableTiming));
            HIPCHK(hipEventRecord(ctx->ev_gate[g], st));
        }
        return 0;
    };
    for (size_t si = 0; si < stages.size(); ++si) {
        const std::vector<uint32_t>& stage = stages[si];
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t nj = group_off[g + 1] - group_off[g];
            if (nj == 0) continue;
            const uint32_t* gjobs = D.jobs + group_off[g];
            hipStream_t s0 = ls[g * W];
            if (stage.size() > 1) {                          // the stage's extra lanes start after the group's previous stop rule
                HIPCHK(hipEventRecord(ctx->ev_fork[g * W], s0));
                for (uint32_t j = 1; j < stage.size(); ++j) HIPCHK(hipStreamWaitEvent(ls[g * W + j], ctx->ev_fork[g * W], 0));
            }
            for (uint32_t jj = 0; jj < stage.size(); ++jj) {
                const uint32_t j = jj;
                const uint32_t p = stage[j], lane = g * W + j;
                const PloidyPlan& q = plan[p];
                hipStream_t st = ls[lane];
                uint32_t* gqueue = D.queue + 2 * ((size_t)lane * P + (p - 1));     // [0] beam, [1] optimise: one counter pair per (lane, ploidy), zeroed once before the
                                                                                    // loop (a memset between persistent launches is a fill KERNEL that waits for wave slots)
                uint8_t* lane_part = D.beam_part + (uint64_t)j * (tot_reads + 16);
                // ---- beam search -----------------------------------------------------------------------------------------
                const bool tail_here = tail_p && p == tail_p;          // this ploidy's beam launch was queued with the stage below: join it
                if (tail_here) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_tail_join[g], 0)); lane_part = tail_part; }
                else if (!q.shortcut) { const int brc = beam_launch(stage, g, nj, gjobs, p, lane, st, gqueue, lane_part, 0); if (brc) return brc; }
                if (tail_p && p + 1 == tail_p) {                         // the fork point: behind this ploidy's beam launch, before its optimise launch
                    if (!ctx->ev_tail[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_tail[g], hipEventDisableTiming));
                    HIPCHK(hipEventRecord(ctx->ev_tail[g], st));
                }
                // ---- optimise + MEC stats ------------------------------------------------------------------------------
                {
                    const uint32_t slots = std::min(q.opt_slots, nj);
                    fl::OptArgs a{};
                    a.bs = bs; a.job_block = gjobs; a.n_jobs = nj; a.ploidy = p; a.max_ploidy = P; a.span_max = span_max; a.n_max = n_max;
                    a.queue_head = gqueue + 1; a.blk_done = D.done; a.eps = prm->epsilon;
                    a.part_in = lane_part; a.part_out = D.planes + (uint64_t)(p - 1) * tot_reads;
                    a.hist_pool = (uint64_t*)(ctx->opt_hist.as<char>() + sl.ohist * lane); a.dist_pool = (double*)(ctx->opt_dist.as<char>() + sl.odist * lane);
                    a.cand_gain_pool = (uint64_t*)(ctx->opt_gain.as<char>() + sl.ogain * lane); a.cand_key_pool = (uint32_t*)(ctx->opt_key.as<char>() + sl.okey * lane);
                    a.moves_pool = (uint32_t*)(ctx->opt_moves.as<char>() + sl.omoves * lane); a.cand_cap = q.cand_cap;
                    a.mec = D.mec; a.num_alleles = D.na; a.iters = D.iters;
                    a.prof = (unsigned long long*)(D.diag + 4);
                    a.fuse_select = stage.size() == 1 ? 1 : 0;
                    a.stopping_heuristic = prm->stopping_heuristic; a.mec_threshold = mec_threshold(prm, p);
                    a.blk_done_w = D.done; a.best_ploidy = D.best; a.tried = D.tried;
                    a.release_tried = tail_p != 0 ? 1u : 0u;
                    a.with_p1 = p1_fused && p == 2 ? 1u : 0u;
                    a.pm_lds_off = q.pm_lds_off;
                    a.w24 = ctx->d_w24.as<uint32_t>();
                    a.opt_delta = K.opt_delta; a.delta_stat = D.diag + 2;          // (diag[2], diag[3]: delta passes run / passes with flips that took the interval pass)
                    // (a plan with ANY speculative stage publishes ready bits and stop_at from every stage: a later stage's stop rule compares with these MEC values)
                    if (K.arith) {
                        a.cell_ord = ctx->cur_ord; a.cell_ord_off = ctx->cur_ord_off;
                        char* base = ctx->arith_pool.as<char>() + sl.arith * lane;
                        a.sort_cap = sort_cap_of(p, span_max); a.fx_ctrl = fx_ctrl; a.fx_slot = fx_slot; a.fx_lds_off = q.fx_lds_off; a.fx_tags = q.fx_tags; a.fx_replay = K.arith_replay; a.fk_lds_off = q.fk_lds_off;
                        a.fk_pool = (uint64_t*)base; base += (uint64_t)slots * p * span_max * 8;
                        a.sk_pool = (uint64_t*)base; base += (uint64_t)slots * a.sort_cap * 8;
                        a.sp_pool = (uint32_t*)base; base += ((uint64_t)slots * a.sort_cap * 4 + 15) & ~(uint64_t)15;
                        a.fx_pool = (uint8_t*)base; base += (((uint64_t)slots * p * 2 * fx_bytes) + 15) & ~(uint64_t)15;
                        a.ol_pool = (uint32_t*)base;
                    }
                    if (W > 1) { a.stop_at = D.stop; a.ready = D.ready; for (uint32_t q2 = 2; q2 <= P; ++q2) a.thresholds[q2] = mec_threshold(prm, q2); }
                    int t = T.begin(K_OPT, st);
                    const hipError_t le = launch_optimize<A>(q, K, slots, st, a);
                    T.end(t);
                    if (le != hipSuccess) return fail(FLORIA_E_DEVICE, std::string("optimize_kernel launch: ") + hipGetErrorString(le));
                    ctx->timing.optimize_launches++;
                    if (q.opt_spec && q.opt_pk && !K.arith) ctx->timing.optimize_packed_launches++;
                }
                if (tail_p && p + 1 == tail_p) {          // (queued AFTER the optimise launch it depends on: streams that share a hardware queue then still make progress)
                    if (!ctx->tstream[g]) HIPCHK(hipStreamCreateWithFlags(&ctx->tstream[g], hipStreamNonBlocking));
                    if (!ctx->ev_tail_join[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_tail_join[g], hipEventDisableTiming));
                    HIPCHK(hipStreamWaitEvent(ctx->tstream[g], ctx->ev_tail[g], 0));
                    const int brc = beam_launch(stages.back(), g, nj, gjobs, tail_p, lane, ctx->tstream[g], D.queue + 2 * ((size_t)lane * P + (tail_p - 1)), tail_part, p);
                    if (brc) return brc;
                    HIPCHK(hipEventRecord(ctx->ev_tail_join[g], ctx->tstream[g]));
                }
            }
            // join the stage's extra lanes, then the stop rule for the stage's ploidies in ascending order (graph_processing.rs:198-251)
            for (uint32_t j = 1; j < stage.size(); ++j) { HIPCHK(hipEventRecord(ctx->ev_join[g * W + j], ls[g * W + j])); HIPCHK(hipStreamWaitEvent(s0, ctx->ev_join[g * W + j], 0)); }
            for (uint32_t j = 0; j < stage.size() && stage.size() > 1; ++j) {                  // (a one-ploidy stage decided inside optimize_kernel)
                const uint32_t p = stage[j];
                fl::SelectArgs s{};
                s.job_block = gjobs; s.n_jobs = nj; s.ploidy = p; s.max_ploidy = P; s.stopping_heuristic = prm->stopping_heuristic; s.eps = prm->epsilon;
                s.mec_threshold = mec_threshold(prm, p);
                s.mec = D.mec; s.num_alleles = D.na; s.iters = D.iters; s.blk_done = D.done; s.best_ploidy = D.best; s.tried = D.tried;
                s.clear_from = (j + 1 == stage.size()) ? 1 : 0;      // last select of a speculative stage: forget the ploidies beyond `tried`
                s.stage_last = stage.back();
                int t = T.begin(K_SEL, s0);
                hipLaunchKernelGGL(fl::select_kernel, dim3((nj + 255) / 256), dim3(256), 0, s0, s);
                T.end(t);
                HIPCHK(hipGetLastError());
            }
        }
    }
    // join: the main stream continues after every group
    for (uint32_t g = 1; g < G; ++g) { HIPCHK(hipEventRecord(ctx->ev_join[g * W], ls[g * W])); HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[g * W], 0)); }
    T.end(t_phase);
    ctx->timing.streams = G;
    ctx->timing.stage_width = W;
    return 0;
}

}  // namespace

// =====================================================================================================
extern "C" {

const char* floria_hip_last_error(void) { return g_err.c_str(); }

}  // extern "C"

// HIP reads GPU_MAX_HW_QUEUES once, when the runtime initialises (lazily, at the first API call); the launch plans of s1_core want 12 hardware queues (below).
// The library does NOT touch the environment on its own (rounds 2-4 did, from a constructor: a setenv() in a process that other threads may be reading the
// environment of): a host either exports GPU_MAX_HW_QUEUES=12 itself or calls floria_hip_init_env() once, from its main thread, before its first HIP
// call; a host that did neither is noticed (probe_hw_queues) and gets plans that stay within the queues it has, with one message on stderr.
extern "C" int floria_hip_init_env(void) { return setenv("GPU_MAX_HW_QUEUES", "12", 0) == 0 ? 0 : FLORIA_E_INVALID; }      // (never overrides a value the user has set)

namespace {
// How many streams of this process really execute side by side?  HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the environment
// said otherwise BEFORE the runtime initialised — a host that touched HIP earlier cannot fix it afterwards), and streams that share a queue run one
// after the other.  The launch plans of s1_core put job groups and the ploidies of a speculative stage on separate streams that WAIT ON EACH OTHER'S
// EVENTS; with fewer queues than lanes they serialise (measured: 3-8x slower) instead of failing.  So the context measures it once: one wave that spins
// for 1 ms, alone and then on 12 fresh streams at once; 12 x (time alone) / (time together) is the number of lanes that ran concurrently.
__global__ void spin_kernel(unsigned long long ticks, unsigned* sink) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (sink && threadIdx.x == 1234567) *sink = 1;
}
uint32_t probe_hw_queues(floria_hip_ctx* c) {
    constexpr int NS = 12;
    hipStream_t st[NS] = {};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint32_t result = 0;
    bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    for (int i = 0; i < NS && ok; ++i) ok = hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking) == hipSuccess;
    const unsigned long long ticks = 100000;         // 1 ms of the 100 MHz wall clock: long against the ~10 us the host needs per launch, so the 12 spins overlap if they can
    auto timed = [&](int n) -> float {
        float ms = 0.f;
        if (hipEventRecord(e0, c->stream) != hipSuccess) return -1.f;
        for (int i = 0; i < n; ++i) { (void)hipStreamWaitEvent(st[i], e0, 0); hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st[i], ticks, (unsigned*)nullptr); }
        for (int i = 0; i < n; ++i) { (void)hipEventRecord(e1, st[i]); (void)hipStreamWaitEvent(c->stream, e1, 0); }
        if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
        return ms;
    };
    if (ok) {
        (void)timed(1);                              // (first launch: code object load)
        const float t1 = timed(1), tn = timed(NS);
        if (t1 > 0.f && tn > 0.f) result = (uint32_t)std::max(1.0f, std::min((float)NS, (float)NS * t1 / tn + 0.35f));
    }
    for (int i = 0; i < NS; ++i) if (st[i]) (void)hipStreamDestroy(st[i]);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipGetLastError();
    return result ? result : 4;                      // (probe failed: assume the runtime's default)
}
}  // namespace

extern "C" {
const char* floria_hip_version(void) { return "floria_hip 0.1.0 (gfx950)"; }

int floria_hip_create(int device, floria_hip_ctx** out) {
    if (!out) return fail(FLORIA_E_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(FLORIA_E_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(FLORIA_E_INVALID, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    floria_hip_ctx* c = new floria_hip_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(FLORIA_E_DEVICE, "hipStreamCreate failed"); }
    // phred_scale (utils_frags.rs:702-711): w = 1f32 - 10f32.powf(q as f32 / -10.), exact multiple of 2^-24
    uint32_t w24[256];
    if (!fl::w24_table(w24)) { delete c; return fail(FLORIA_E_DEVICE, "quality weight is not a multiple of 2^-24"); }
    memcpy(c->w24, w24, sizeof(w24));
    uint64_t s = 0xf10a1a2024ull;
    for (int k = 0; k < FLORIA_MAX_PLOIDY; ++k) { c->Rk1[k] = splitmix64(s) | 1ull; c->Rk2[k] = splitmix64(s) | 1ull; }
    e = hipMemcpyToSymbol(HIP_SYMBOL(fl::c_rk1), c->Rk1, sizeof(c->Rk1));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(fl::c_rk2), c->Rk2, sizeof(c->Rk2));
    if (e != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return fail(FLORIA_E_DEVICE, std::string("hash multiplier upload: ") + hipGetErrorString(e)); }
    if (int rc = ensure_hash(c, 4 * fl::HASH_M)) { (void)hipStreamDestroy(c->stream); delete c; return rc; }
    if (c->d_w24.ensure(sizeof(w24)) || hipMemcpy(c->d_w24.p, w24, sizeof(w24), hipMemcpyHostToDevice) != hipSuccess) { floria_hip_destroy(c); return fail(FLORIA_E_DEVICE, "weight table upload failed"); }
    {   // development knobs: environment defaults, read once (floria_hip_set_option overrides them)
        Knobs& K = c->knobs;
        if (const char* v = getenv("FLORIA_HIP_GROUPS")) K.groups = (uint32_t)std::max(0, std::min<int>(atoi(v), floria_hip_ctx::MAX_GROUPS));
        if (const char* v = getenv("FLORIA_HIP_BEAM")) K.beam_path = !strcmp(v, "generic") ? 1 : !strcmp(v, "slab") ? 2 : !strcmp(v, "wide") ? 3 : 0;
        K.no_specialized = getenv("FLORIA_HIP_NO_SPECIALIZED") != nullptr;
        K.no_p1_shortcut = getenv("FLORIA_HIP_NO_P1_SHORTCUT") != nullptr;
        if (const char* v = getenv("FLORIA_HIP_OPT_THREADS")) { const int tv = atoi(v); if (tv == 1024 || tv == 512 || tv == 128) K.opt_threads = (uint32_t)tv; }
        K.opt_global = getenv("FLORIA_HIP_OPT_GLOBAL") != nullptr;
        K.opt_block_order = getenv("FLORIA_HIP_OPT_BLOCK_ORDER") != nullptr;
        if (const char* v = getenv("FLORIA_HIP_OPT_PACKED")) K.opt_packed = atoi(v) != 0;
        if (const char* v = getenv("FLORIA_HIP_OPT_DELTA")) K.opt_delta = atoi(v) != 0;
        if (const char* v = getenv("FLORIA_HIP_SPECULATE")) K.speculate = std::max(-1, std::min(3, atoi(v)));
        K.trace = getenv("FLORIA_HIP_TRACE") != nullptr;
        if (const char* v = getenv("FLORIA_HIP_TAIL_OVERLAP")) K.tail_overlap = std::max(-1, std::min(1, atoi(v)));
        if (const char* v = getenv("FLORIA_HIP_FUSE_P1")) K.fuse_p1 = std::max(-1, std::min(1, atoi(v)));
        if (const char* v = getenv("FLORIA_HIP_TAIL_WAVES")) K.tail_waves = (uint32_t)std::max(1, std::min(16, atoi(v)));
        if (const char* v = getenv("FLORIA_HIP_SPEC_GATE_DIV")) K.spec_gate_div = (uint32_t)std::max(1, std::min(16, atoi(v)));
        if (const char* v = getenv("FLORIA_HIP_STAGE_THREADS")) c->stage_threads = (uint32_t)std::max(1, std::min(16, atoi(v)));
        else c->stage_threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    }
    c->hw_queues = probe_hw_queues(c);
    if (const char* v = getenv("FLORIA_HIP_HW_QUEUES")) c->hw_queues = (uint32_t)std::max(1, std::min(64, atoi(v)));      // (measurements under a profiler, which slows the probe's launches down)
    if (c->knobs.trace) fprintf(stderr, "[floria_hip] device %d: %u streams run side by side\n", device, c->hw_queues);
    if (c->hw_queues < 5) {      // (the probe reads 6 with GPU_MAX_HW_QUEUES=12 - two rounds of its 12 spins - and 3-4 with HIP's default of 4 queues - three or four rounds)
        static std::atomic<bool> said{false};
        if (!said.exchange(true))
            fprintf(stderr, "floria_hip: only %u streams of this process run concurrently on device %d (GPU_MAX_HW_QUEUES was not set to 12 before HIP initialised?): "
                            "speculative ploidy stages are off and calls use at most two job groups; small batches will be slower.\n", c->hw_queues, device);
    }
    *out = c;
    return 0;
}

void floria_hip_destroy(floria_hip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    sync_all(c);
    for (DevBuf* b : {&c->d_binom, &c->d_hash, &c->d_w24, &c->state_pool, &c->hist_pool, &c->opt_hist, &c->opt_dist, &c->opt_gain, &c->opt_key, &c->opt_moves, &c->misc, &c->misc0, &c->graph_buf, &c->graph_hist, &c->graph_sort, &c->up_tmp, &c->arith_ord, &c->arith_scr, &c->arith_tab, &c->arith_pool, &c->pile_in, &c->pile_out, &c->asm_plan, &c->asm_ord_scr, &c->mono_buf, &c->span_buf, &c->hs_tmp, &c->join_bits, &c->inf_in, &c->rec_in, &c->rec_out, &c->rec_names, &c->seq_in, &c->seq_out, &c->est_in, &c->est_win, &c->est_cols}) b->release();
    for (Arena* a : c->arena_cache) { a->buf.release(); delete a; }
    c->stage.release();
    c->box.release();
    for (uint32_t g = 0; g < floria_hip_ctx::MAX_LANES; ++g) {
        if (c->gstream[g]) (void)hipStreamDestroy(c->gstream[g]);
        if (c->gstream_low[g]) (void)hipStreamDestroy(c->gstream_low[g]);
        if (g < floria_hip_ctx::MAX_GROUPS && c->ev_gate[g]) (void)hipEventDestroy(c->ev_gate[g]);
        if (g < floria_hip_ctx::MAX_GROUPS && c->ev_tail[g]) (void)hipEventDestroy(c->ev_tail[g]);
        if (g < floria_hip_ctx::MAX_GROUPS && c->ev_tail_join[g]) (void)hipEventDestroy(c->ev_tail_join[g]);
        if (g < floria_hip_ctx::MAX_GROUPS && c->tstream[g]) (void)hipStreamDestroy(c->tstream[g]);
        if (c->ev_join[g]) (void)hipEventDestroy(c->ev_join[g]);
        if (c->ev_fork[g]) (void)hipEventDestroy(c->ev_fork[g]);
    }
    if (c->ev_rids) (void)hipEventDestroy(c->ev_rids);
    for (hipEvent_t e : c->ev_chunk) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_copied) if (e) (void)hipEventDestroy(e);
    if (c->flat_stream) (void)hipStreamDestroy(c->flat_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

// the grid of a grid-stride launch of the resident chain: as computed, unless the test option "chain_wgs" caps it
static inline uint32_t chain_grid(const floria_hip_ctx* ctx, uint32_t grid) {
    const uint32_t cap = ctx->knobs.chain_wgs;
    return cap && grid > cap ? cap : grid;
}
// ... of the chain's usual shape: `per_wg` items per workgroup and trip (4 = one wavefront per item), grid-stride beyond 8 workgroups per CU, one workgroup at the least
static inline uint32_t items_grid(const floria_hip_ctx* ctx, uint64_t items, uint32_t per_wg) {
    return chain_grid(ctx, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_wg - 1) / per_wg, (uint64_t)ctx->n_cu * 8)));
}
// counts[0..n) -> their exclusive prefix sums in place, the total in counts[n] (pileup_kernel.h); `tiles`: a word per PILEUP_SCAN_TILE counts.  The caller asks hipGetLastError.
static inline void launch_offset_scan(const floria_hip_ctx* ctx, uint64_t* counts, uint64_t* tiles, uint32_t n) {
    const uint32_t n_tiles = (n + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
    hipLaunchKernelGGL(fl::pileup_scan_tiles_kernel, dim3(n_tiles), dim3(256), 0, ctx->stream, counts, tiles, n);
    hipLaunchKernelGGL(fl::pileup_scan_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, tiles, n_tiles, counts + n);
    hipLaunchKernelGGL(fl::pileup_scan_add_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, counts, (const uint64_t*)tiles, n);
}

int floria_hip_set_slots(floria_hip_ctx* ctx, uint32_t beam_slots) {
    if (!ctx) return fail(FLORIA_E_INVALID, "null ctx");
    ctx->user_slots = beam_slots;
    return 0;
}

int floria_hip_set_option(floria_hip_ctx* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return fail(FLORIA_E_INVALID, "null argument");
    const std::string k(key);
    Knobs& K = ctx->knobs;
    if (k == "groups") K.groups = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, floria_hip_ctx::MAX_GROUPS));
    else if (k == "beam_path") { if (value < 0 || value > 3) return fail(FLORIA_E_INVALID, "beam_path: 0 auto | 1 generic | 2 slab | 3 wide"); K.beam_path = (uint32_t)value; }
    else if (k == "no_specialized") K.no_specialized = value != 0;
    else if (k == "no_p1_shortcut") K.no_p1_shortcut = value != 0;
    else if (k == "opt_threads") { if (value != 0 && value != 128 && value != 512 && value != 1024) return fail(FLORIA_E_INVALID, "opt_threads: 0 | 128 | 512 | 1024"); K.opt_threads = (uint32_t)value; }
    else if (k == "opt_global") K.opt_global = value != 0;
    else if (k == "spec_gate_div") K.spec_gate_div = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(value, 16));
    else if (k == "speculate") { if (value < -1 || value > 3) return fail(FLORIA_E_INVALID, "speculate: -1 auto | 0 | 1 | 2 | 3"); K.speculate = (int32_t)value; }
    else if (k == "no_bulk") K.no_bulk = value != 0;
    else if (k == "opt_block_order") K.opt_block_order = value != 0;
    else if (k == "opt_packed") K.opt_packed = value != 0;
    else if (k == "opt_delta") K.opt_delta = value != 0;
    else if (k == "tail_overlap") { if (value < -1 || value > 1) return fail(FLORIA_E_INVALID, "tail_overlap: 0 | 1"); K.tail_overlap = (int32_t)value; }
    else if (k == "fuse_p1") { if (value < -1 || value > 1) return fail(FLORIA_E_INVALID, "fuse_p1: -1 auto | 0 | 1"); K.fuse_p1 = (int32_t)value; }
    else if (k == "tail_waves") K.tail_waves = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(value, 16));
    else if (k == "arith_hbm") K.arith_hbm = value != 0;
    else if (k == "arith_replay") { K.arith_replay = value != 0; ctx->ord_epoch = ~0ull; }      // (the cell orders are computed again, the long way or the short one)
    else if (k == "asm_order_general") K.asm_order_general = value != 0;
    else if (k == "chain_wgs") { if (value < 0 || value > (int64_t)0x7fffffff) return fail(FLORIA_E_INVALID, "chain_wgs: 0 off | the largest grid of the resident chain's grid-stride launches"); K.chain_wgs = (uint32_t)value; }
    else if (k == "fx_tags") { if (value != 0 && (value < (int64_t)fl::FX_TAGS_MIN || value > (int64_t)fl::FX_TAGS_MAX || (value & (value - 1)))) return fail(FLORIA_E_INVALID, "fx_tags: 0 | a power of two in 128..1024"); K.fx_tags = (uint32_t)value; }
    else if (k == "arith_ow6") K.arith_ow6 = value != 0;
    else if (k == "s2_assign_only") K.s2_assign_only = value != 0;
    else if (k == "s1_no_lists") K.s1_no_lists = value != 0;
    else if (k == "arith") { if (value < 0 || value > 1) return fail(FLORIA_E_INVALID, "arith: 0 canonical | 1 the reference's running sums"); K.arith = (uint32_t)value; }
    else if (k == "hw_queues") ctx->hw_queues = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(value, 64));      // (tests: pretend the probe found this many)
    else if (k == "upload_chunks") K.upload_chunks = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, floria_hip_ctx::MAX_GROUPS));
    else if (k == "trace") K.trace = value != 0;
    else if (k == "reassign_path") { if (value < 0 || value > 2) return fail(FLORIA_E_INVALID, "reassign_path: 0 auto | 1 parallel | 2 chain"); K.reassign_path = (uint32_t)value; }
    else if (k == "inflate_slots") { if (value < 0 || value > (int64_t)0x7fffffff) return fail(FLORIA_E_INVALID, "inflate_slots: 0 = two members per CU | the largest number of members in flight"); ctx->inflate_slots = (uint32_t)value; }
    else if (k == "estimate_window") { if (value < 0 || value > (int64_t)(1u << 30)) return fail(FLORIA_E_INVALID, "estimate_window: 0 = 2^22 positions | 1 .. 2^30 positions per window"); ctx->estimate_window = (uint32_t)value; }
    else if (k == "slots") ctx->user_slots = (uint32_t)std::max<int64_t>(0, value);
    else if (k == "stage_threads") ctx->stage_threads = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(value, 16));
    else return fail(FLORIA_E_INVALID, "unknown option '" + k + "'");
    return 0;
}

int floria_hip_last_timing(const floria_hip_ctx* ctx, floria_timing* out) {
    if (!ctx || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = ctx->timing;
    return 0;
}

// ---- get_range_with_lengths (utils_frags.rs:405-463) ------------------------------------------------------
int floria_hip_block_ranges(const uint64_t* g, uint32_t n, uint64_t block_length, uint64_t overlap_len,
                            double minimal_density, floria_ranges** out) {
    if (!g || !out) return fail(FLORIA_E_INVALID, "null argument");
    if (n == 0) return fail(FLORIA_E_INVALID, "empty snp_to_genome_pos");
    std::vector<uint32_t> S, E;
    uint64_t cum_pos = 0, last_pos = g[0];
    uint32_t left_endpoint = 0, new_left_end = 0;
    bool hit_new_left = false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t pos = g[i];
        if (i == n - 1) { S.push_back(left_endpoint); E.push_back(i); break; }                         // :418-421
        if (pos < last_pos) return fail(FLORIA_E_INVALID, "VCF malformed. Positions are not increasing");   // :422-425
        cum_pos += pos - last_pos;
        last_pos = pos;
        if (cum_pos > block_length - overlap_len && !hit_new_left) { new_left_end = i; hit_new_left = true; }
        if (cum_pos > block_length) {
            cum_pos = 0;
            const double snp_density = (double)(i - left_endpoint) / (double)block_length;
            if (snp_density > minimal_density) { S.push_back(left_endpoint); E.push_back(i - 1); }
            left_endpoint = (g[new_left_end] + block_length < g[new_left_end + 1]) ? new_left_end : new_left_end + 1;   // :447-453
            last_pos = g[left_endpoint];
            hit_new_left = false;
        }
    }
    floria_ranges* r = (floria_ranges*)calloc(1, sizeof(floria_ranges));
    if (!r) return fail(FLORIA_E_NOMEM, "calloc");
    r->n = (uint32_t)S.size();
    r->start = (uint32_t*)malloc(sizeof(uint32_t) * (S.size() + 1));
    r->end = (uint32_t*)malloc(sizeof(uint32_t) * (S.size() + 1));
    for (size_t i = 0; i < S.size(); ++i) { r->start[i] = S[i] + 1; r->end[i] = E[i] + 1; }   // 1-indexed :461
    *out = r;
    return 0;
}
void floria_hip_ranges_free(floria_ranges* r) { if (r) { free(r->start); free(r->end); free(r); } }

// ---- contig upload ------------------------------------------------------------------------------------------
// Pinned host memory for hosts that marshal their `Vec<Frag>` straight into upload buffers: arrays that live here go to the
// device by DMA with no staging copy.
void* floria_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); fail(FLORIA_E_NOMEM, "hipHostMalloc failed"); return nullptr; }
    return p;
}
void floria_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }

}  // extern "C"

namespace {

bool is_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// One host->device transfer plan entry: `bytes` from `src` to `dst` (contiguous on both sides).
struct CopyRun { const char* src; char* dst; size_t bytes; };

int issue_copies(floria_hip_ctx* ctx, std::vector<CopyRun>& runs, uint64_t* pinned_bytes, uint64_t* staged_bytes);

Arena* arena_get(floria_hip_ctx* ctx, size_t bytes);
void arena_put(Arena* a);

int host_meta(const floria_hip_contig* cc) {
    floria_hip_contig* c = const_cast<floria_hip_contig*>(cc);
    Arena* a = c->arena;
    if (!a->host_meta) {
        a->h_first.resize(a->R + 1); a->h_last.resize(a->R + 1);
        if (a->R) {
            HIPCHK(hipMemcpy(a->h_first.data(), a->buf.as<char>() + a->off_first, 4 * a->R, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(a->h_last.data(), a->buf.as<char>() + a->off_last, 4 * a->R, hipMemcpyDeviceToHost));
        }
        a->host_meta = true;
    }
    c->h_first = a->h_first.data() + a->read_prefix[c->idx];
    c->h_last = a->h_last.data() + a->read_prefix[c->idx];
    return 0;
}

}  // namespace

extern "C" {

}  // extern "C"

namespace {

// Where the regions of a batch arena lie, for R reads and C cells in n contigs.  There is one definition, and one builder (UploadPlan::open below) that every producer
// of resident contigs goes through (plan_upload, floria_hip_assemble_contigs, floria_hip_drop_monomorphic), so that their handles cannot differ in layout.  16-B tails:
// the beam kernel's LDS-DMA moves cells in 16-B pieces.  The set-order region exists only when some contig carries one, the seq_pos region only when some contig carries
// positions; it lies behind every other region, so no other offset depends on it.
struct ArenaLayout { size_t o_ro = 0, o_first = 0, o_last = 0, o_snp = 0, o_aw = 0, o_tw = 0, o_meta = 0, o_so = 0, o_sp = 0, o_pk = 0, bytes = 0; bool pk = false; };
ArenaLayout layout_arena(uint64_t R, uint64_t C, uint32_t n, bool any_so, bool any_sp, bool pk) {
    ArenaLayout Y;
    Carve X;
    Y.o_ro = X.seg(4 * (R + n)).off; Y.o_first = X.seg(4 * R).off; Y.o_last = X.seg(4 * R).off; Y.o_snp = X.seg(4 * C + 16).off; Y.o_aw = X.seg(4 * C + 16).off;
    Y.o_tw = X.seg(16 * R).off; Y.o_meta = X.seg(32 * R).off;
    Y.o_so = any_so ? X.seg(4 * C + 16).off : 0;
    Y.o_sp = any_sp ? X.seg(4 * C + 16).off : 0;
    // the packed cells (common.h): optimize_kernel reads them in aligned 16-B pieces, which may reach up to 12 bytes before a contig's first and behind its last cell -
    // into the neighbouring contig's cells, or into the region's own head (256-B aligned) and tail (the 16 bytes here)
    Y.pk = pk; Y.o_pk = pk ? X.seg(4 * C + 16).off : 0;
    Y.bytes = X.cursor;
    return Y;
}
// ... and contig i's views into them (rp / cp: reads / cells before every contig)
void arena_contig(const ArenaLayout& Y, char* D, const std::vector<uint64_t>& rp, const std::vector<uint64_t>& cp, uint32_t i, fl::UploadContig& u) {
    u.read_off = (const uint32_t*)(D + Y.o_ro + 4 * (rp[i] + i)); u.first = (const uint32_t*)(D + Y.o_first + 4 * rp[i]); u.last = (const uint32_t*)(D + Y.o_last + 4 * rp[i]);
    u.snp = (const uint32_t*)(D + Y.o_snp + 4 * cp[i]); u.cell_aw = (uint32_t*)(D + Y.o_aw + 4 * cp[i]); u.cell_pk = Y.pk ? (uint32_t*)(D + Y.o_pk + 4 * cp[i]) : nullptr; u.tw = (uint64_t*)(D + Y.o_tw + 16 * rp[i]); u.meta = (uint32_t*)(D + Y.o_meta + 32 * rp[i]);
    u.n_reads = (uint32_t)(rp[i + 1] - rp[i]); u.n_cells = (uint32_t)(cp[i + 1] - cp[i]);
}

// A batch of resident contigs under construction, and the one owner of its arena until the handles take it over.  open() does what every producer needs, in this order:
// the upload epoch moves on, the batch is one chunk, the arena is laid out, taken and described, the transient tables of the validate + flatten launch (and, with
// `raw`, the raw allele / qual bytes it reads) are placed in up_tmp, and every contig gets its views and a fresh status word.  What differs per contig stays with the
// producer, as one loop over so_dev / sp_dev behind open().  commit() turns the status words into an error or into the handles; unless it succeeded, the destructor
// waits for the device (sync_all), gives the arena back and nulls the caller's handles — so every error path below is a plain return.
// For a host upload the plan also says which host->device transfers carry the arrays (arrays of consecutive contigs that are back to back in host memory merge into
// one transfer).  The cell arrays (snp, allele, qual — 99 % of the bytes) are planned per CHUNK of consecutive contigs, so that a caller can start work on chunk g
// while chunk g+1 is still on the wire (floria_hip_phase_pileups_batch).
struct UploadPlan {
    floria_hip_ctx* ctx = nullptr;
    floria_hip_contig** out = nullptr;                  // [n] the caller's handles
    uint32_t n = 0, n_chunks = 1;
    std::vector<uint64_t> rp, cp;                       // read / cell prefix per contig
    uint64_t R = 0, C = 0;
    Arena* A = nullptr;                                 // (null again once the handles own it)
    ArenaLayout Y;
    char *D = nullptr, *T = nullptr;                    // arena base, transient base
    size_t t_al = 0, t_q = 0, t_cd = 0, t_rp = 0, t_st = 0, t_more = 0;      // transient: raw alleles, raw quals, contig table, read prefix, status words, the caller's own bytes
    std::vector<fl::UploadContig> ucd;
    std::vector<fl::UploadStatus> ust;
    std::vector<fl::PackedContig> upk;                  // packed uploads: what expand_kernel reads / writes (device table at t_pk)
    size_t t_pk = 0;
    bool packed = false;
    std::vector<CopyRun> small_runs;                    // read_off, first, last (packed: + bit_off) of every contig
    std::vector<std::vector<CopyRun>> chunk_runs;       // snp, allele, qual per chunk
    std::vector<uint32_t> chunk_first;                  // [n_chunks+1] contig boundaries
    std::vector<uint32_t> contig_chunk;                 // [n]
    std::vector<const uint32_t*> so_dev;                // [n] device copy of the contig's set_order (include/floria_hip.h), null where it has none
    std::vector<const uint32_t*> sp_dev;                // [n] the contig's part of the seq_pos region, null where it carries no positions (empty: none does)
    bool all_pinned = false;

    UploadPlan() = default;
    UploadPlan(const UploadPlan&) = delete;
    UploadPlan& operator=(const UploadPlan&) = delete;
    ~UploadPlan() { if (A) { sync_all(ctx); release(); for (uint32_t i = 0; out && i < n; ++i) out[i] = nullptr; } }
    void release() { arena_put(A); A = nullptr; }      // (back to the cache without a wait: nothing was issued yet)
    uint32_t* so_at(uint32_t i) const { return (uint32_t*)(D + Y.o_so + 4 * cp[i]); }      // where contig i's set order / positions lie if it carries them
    uint32_t* sp_at(uint32_t i) const { return (uint32_t*)(D + Y.o_sp + 4 * cp[i]); }
    fl::ContigDev dev(uint32_t i) const { const fl::UploadContig& u = ucd[i]; return fl::ContigDev{u.read_off, u.first, u.last, u.snp, u.cell_aw, u.tw, u.meta, u.n_reads, 0, so_dev[i], u.cell_pk}; }      // what the kernels see of contig i
    // `raw`: the flatten launch reads raw allele / qual bytes from up_tmp (a host upload's DMA or assemble's FILL puts them there), and its tables lie behind them, with
    // `more` bytes of the caller's at t_more.  Without it nothing of up_tmp is touched: the producer writes the resident form and keeps the tables where it likes.
    int open(floria_hip_ctx* c, uint32_t n_contigs, std::vector<uint64_t> read_prefix, std::vector<uint64_t> cell_prefix, bool any_so, bool any_sp, floria_hip_contig** handles,
             bool raw, size_t more = 0, bool with_pk = false) {
        ctx = c; out = handles; n = n_contigs; rp = std::move(read_prefix); cp = std::move(cell_prefix); R = rp[n]; C = cp[n];
        ctx->upload_epoch++;                               // (device memory of contigs is about to be rewritten: cached cell orders no longer describe it)
        n_chunks = 1; chunk_first = {0, n}; contig_chunk.assign(n, 0);
        Y = layout_arena(R, C, n, any_so, any_sp, with_pk && raw);      // (packed cells are written by flatten_kernel, from the raw quality bytes)
        A = arena_get(ctx, Y.bytes + 256);
        if (!A) return FLORIA_E_NOMEM;
        A->n_contigs = n; A->R = R; A->C = C; A->off_ro = Y.o_ro; A->off_first = Y.o_first; A->off_last = Y.o_last; A->read_prefix = rp; A->host_meta = false;
        D = A->buf.as<char>();
        if (raw) {
            Carve X;
            const Seg s_al = X.seg(C + 16), s_q = X.seg(C + 16), s_cd = X.seg(sizeof(fl::UploadContig) * n), s_rp = X.seg(8ull * (n + 1)), s_st = X.seg(sizeof(fl::UploadStatus) * n), s_more = X.seg(more);
            if (int rc = X.place(ctx->up_tmp)) return rc;
            T = X.base; t_al = s_al.off; t_q = s_q.off; t_cd = s_cd.off; t_rp = s_rp.off; t_st = s_st.off; t_more = s_more.off;
        }
        ucd.resize(n); ust.resize(n); so_dev.assign(n, nullptr);
        if (any_sp) sp_dev.assign(n, nullptr);
        for (uint32_t i = 0; i < n; ++i) {
            fl::UploadContig& u = ucd[i];
            arena_contig(Y, D, rp, cp, i, u);
            u.allele = raw ? (const uint8_t*)(T + t_al + cp[i]) : nullptr; u.qual = raw ? (const uint8_t*)(T + t_q + cp[i]) : nullptr;
            ust[i] = fl::UploadStatus{~0ull, 0, 0, 0, 0};
        }
        return 0;
    }
    int commit();
};

// (a batch is either CSR pileups or packed ones: `pk` non-null selects the compact wire form, expanded on the device)
int plan_upload(floria_hip_ctx* ctx, const floria_pileup* pileups, const floria_pileup_packed* pk, uint32_t n, uint32_t n_chunks, floria_hip_contig** out, UploadPlan& P) {
    std::vector<uint64_t> rp(n + 1, 0), cp(n + 1, 0);
    std::vector<floria_pileup> views;                   // packed: the fields both forms share, so that the code below reads one type
    if (pk) {
        views.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            const floria_pileup_packed* q = &pk[i];
            if (q->n_reads && (!q->read_off || !q->first || !q->last || !q->bit_off || !q->present || !q->allele2 || !q->qual)) return fail(FLORIA_E_INVALID, "null pileup field");
            views[i] = floria_pileup{q->read_off, nullptr, nullptr, q->qual, q->first, q->last, q->n_reads, q->set_order};
        }
        pileups = views.data();
    }
    for (uint32_t i = 0; i < n; ++i) {
        const floria_pileup* p = &pileups[i];
        if (!pk && p->n_reads && (!p->read_off || !p->snp || !p->allele || !p->qual || !p->first || !p->last)) return fail(FLORIA_E_INVALID, "null pileup field");
        const uint64_t nc = p->n_reads ? p->read_off[p->n_reads] : 0;
        if (nc >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "more than 2^32 cells in one contig");
        rp[i + 1] = rp[i] + p->n_reads; cp[i + 1] = cp[i] + nc;
    }
    bool any_so = false;                                                                                // host-given set orders (optional, the reference-arithmetic mode reads them)
    for (uint32_t i = 0; i < n; ++i) any_so = any_so || (pileups[i].n_reads && pileups[i].set_order);
    // packed: the compact arrays are transient too (bit offsets, presence bits, 2-bit alleles), one sub-range per contig — at the offsets
    // floria_hip_pack_pileups_batch gives them in host memory, so that a batch packed by it travels as one transfer per field and chunk
    std::vector<uint64_t> pb(n + 1, 0);                 // presence bytes prefix
    Carve X;                                            // (offsets inside the plan's t_more bytes)
    Seg s_bo{}, s_pr{}, s_a2{}, s_pk{};
    if (pk) {
        for (uint32_t i = 0; i < n; ++i) pb[i + 1] = pb[i] + (pk[i].n_reads ? ((uint64_t)pk[i].bit_off[pk[i].n_reads] + 7) / 8 : 0) + 1;
        s_bo = X.seg(4 * (rp[n] + n)); s_pr = X.seg(pb[n] + 16); s_a2 = X.seg(cp[n] / 4 + n + 16); s_pk = X.seg(sizeof(fl::PackedContig) * n);
    }
    P.packed = pk != nullptr;
    if (int rc = P.open(ctx, n, std::move(rp), std::move(cp), any_so, false, out, true, X.cursor, true)) return rc;      // (uploads carry no positions)
    const uint64_t C = P.C;
    const size_t o_ro = P.Y.o_ro, o_first = P.Y.o_first, o_last = P.Y.o_last, o_snp = P.Y.o_snp, t_al = P.t_al, t_q = P.t_q;
    const size_t t_bo = P.t_more + s_bo.off, t_pr = P.t_more + s_pr.off, t_a2 = P.t_more + s_a2.off;
    P.t_pk = P.t_more + s_pk.off;
    char *D = P.D, *T = P.T;
    // chunks: consecutive contigs, balanced by cells
    n_chunks = std::max<uint32_t>(1, std::min<uint32_t>(n_chunks, n));
    P.n_chunks = n_chunks;
    P.chunk_first.assign(n_chunks + 1, n); P.chunk_first[0] = 0;
    P.contig_chunk.assign(n, 0);
    {
        // chunk weights: a small first chunk puts the GPU to work early, a small last chunk keeps the chain that starts last short
        std::vector<double> cum(n_chunks + 1, 0.0);
        for (uint32_t g = 0; g < n_chunks; ++g) {
            const double w = (n_chunks >= 2 && g == 0) ? 0.5 : 1.0;          // (a half-size first chunk measured best)
            cum[g + 1] = cum[g] + w;
        }
        uint32_t g = 0;
        for (uint32_t i = 0; i < n; ++i) {
            while (g + 1 < n_chunks && (double)P.cp[i] >= (double)C * cum[g + 1] / cum[n_chunks] && i > P.chunk_first[g]) P.chunk_first[++g] = i;
            P.contig_chunk[i] = g;
        }
        for (uint32_t h = g + 1; h < n_chunks; ++h) P.chunk_first[h] = n;          // (fewer non-empty chunks than asked for)
    }
    // ---- the transfers ---------------------------------------------------------------------------------------------------------
    auto add_run = [](std::vector<CopyRun>& runs, const void* src, char* dst, size_t bytes) {
        if (!bytes) return;
        // back to back on both sides — or separated by the same few padding bytes on both sides (the field-major layout of floria_hip_pack_pileups_batch
        // pads every contig's bit arrays by a byte): one transfer
        const ptrdiff_t gs = runs.empty() ? -1 : (const char*)src - (runs.back().src + runs.back().bytes), gd = runs.empty() ? -2 : dst - (runs.back().dst + runs.back().bytes);
        if (gs == gd && gs >= 0 && gs <= 64) runs.back().bytes += (size_t)gs + bytes;
        else runs.push_back({(const char*)src, dst, bytes});
    };
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t i = 0; i < n; ++i) {
            const floria_pileup* p = &pileups[i];
            if (!p->n_reads) continue;
            const uint64_t nr = p->n_reads;
            if (kind == 0) add_run(P.small_runs, p->read_off, D + o_ro + 4 * (P.rp[i] + i), 4 * (nr + 1));
            else if (kind == 1) add_run(P.small_runs, p->first, D + o_first + 4 * P.rp[i], 4 * nr);
            else add_run(P.small_runs, p->last, D + o_last + 4 * P.rp[i], 4 * nr);
        }
    if (pk) for (uint32_t i = 0; i < n; ++i) if (pk[i].n_reads) add_run(P.small_runs, pk[i].bit_off, T + t_bo + 4 * (P.rp[i] + i), 4 * ((size_t)pk[i].n_reads + 1));
    auto a2_off = [&](uint32_t i) { return (size_t)(P.cp[i] / 4 + i); };       // (every contig's 2-bit array starts on its own byte)
    P.chunk_runs.assign(n_chunks, {});
    for (uint32_t g = 0; g < n_chunks; ++g)
        for (int kind = 0; kind < 4; ++kind)
            for (uint32_t i = P.chunk_first[g]; i < P.chunk_first[g + 1]; ++i) {
                const floria_pileup* p = &pileups[i];
                if (!p->n_reads) continue;
                const uint64_t nc = P.cp[i + 1] - P.cp[i];
                if (kind == 3) { if (p->set_order) add_run(P.chunk_runs[g], p->set_order, (char*)P.so_at(i), 4 * nc); continue; }
                if (pk) {
                    if (kind == 0) add_run(P.chunk_runs[g], pk[i].present, T + t_pr + pb[i], pb[i + 1] - pb[i] - 1);
                    else if (kind == 1) add_run(P.chunk_runs[g], pk[i].allele2, T + t_a2 + a2_off(i), (nc + 3) / 4);
                    else add_run(P.chunk_runs[g], p->qual, T + t_q + P.cp[i], nc);
                    continue;
                }
                if (kind == 0) add_run(P.chunk_runs[g], p->snp, D + o_snp + 4 * P.cp[i], 4 * nc);
                else if (kind == 1) add_run(P.chunk_runs[g], p->allele, T + t_al + P.cp[i], nc);
                else add_run(P.chunk_runs[g], p->qual, T + t_q + P.cp[i], nc);
            }
    for (uint32_t i = 0; i < n; ++i) if (pileups[i].n_reads && pileups[i].set_order) P.so_dev[i] = P.so_at(i);
    if (pk) {
        P.upk.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            fl::PackedContig& q = P.upk[i];
            q.bit_off = (const uint32_t*)(T + t_bo + 4 * (P.rp[i] + i)); q.present = (const uint8_t*)(T + t_pr + pb[i]); q.allele2 = (const uint8_t*)(T + t_a2 + a2_off(i));
            q.snp = (uint32_t*)(D + o_snp + 4 * P.cp[i]); q.allele = (uint8_t*)(T + t_al + P.cp[i]);
            q.present_bytes = pk[i].n_reads ? ((uint64_t)pk[i].bit_off[pk[i].n_reads] + 7) / 8 : 0;
        }
    }
    P.all_pinned = true;
    auto pinned_run = [](const CopyRun& r) { return r.bytes < 4096 || (is_pinned(r.src) && is_pinned(r.src + r.bytes - 1)); };
    for (auto& r : P.small_runs) P.all_pinned = P.all_pinned && pinned_run(r);
    for (auto& v : P.chunk_runs) for (auto& r : v) P.all_pinned = P.all_pinned && pinned_run(r);
    return 0;
}

// the flatten kernel's tables (contig table, read prefix, fresh status words) — before any flatten launch
hipError_t issue_tables(floria_hip_ctx* ctx, UploadPlan& P, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(P.T + P.t_cd, P.ucd.data(), sizeof(fl::UploadContig) * P.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(P.T + P.t_rp, P.rp.data(), 8 * (P.n + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(P.T + P.t_st, P.ust.data(), sizeof(fl::UploadStatus) * P.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && P.packed) e = hipMemcpyAsync(P.T + P.t_pk, P.upk.data(), sizeof(fl::PackedContig) * P.n, hipMemcpyHostToDevice, st);
    return e;
}
// validate + flatten the reads of chunk g (its cells and the small arrays must have arrived on `st`)
hipError_t launch_flatten(floria_hip_ctx* ctx, UploadPlan& P, uint32_t g, hipStream_t st) {
    const uint32_t c0 = P.chunk_first[g], c1 = P.chunk_first[g + 1];
    const uint64_t nr = P.rp[c1] - P.rp[c0];
    if (!nr) return hipSuccess;
    fl::UploadArgs a{};
    a.contigs = (const fl::UploadContig*)(P.T + P.t_cd) + c0; a.read_prefix = (const uint64_t*)(P.T + P.t_rp) + c0; a.status = (fl::UploadStatus*)(P.T + P.t_st) + c0;
    a.w24 = ctx->d_w24.as<uint32_t>(); a.Rq1 = ctx->d_hash.as<uint64_t>(); a.Rq2 = ctx->d_hash.as<uint64_t>() + 2ull * ctx->hash_len;
    a.n_contigs = c1 - c0; a.read_base = P.rp[c0]; a.n_reads_total = nr;
    const unsigned wgs = (unsigned)((nr + fl::UP_READS_PER_WG - 1) / fl::UP_READS_PER_WG);
    if (P.packed) hipLaunchKernelGGL(fl::expand_kernel, dim3(wgs), dim3(64), 0, st, a, (const fl::PackedContig*)(P.T + P.t_pk) + c0);     // compact wire form -> CSR, then as usual
    hipLaunchKernelGGL(fl::flatten_kernel, dim3(wgs), dim3(64), 0, st, a);
    return hipGetLastError();
}
// status words -> error (if any), else the contig handles, which own the arena from here on
int UploadPlan::commit() {
    const UploadPlan& P = *this;
    for (uint32_t i = 0; i < n; ++i) if (P.ust[i].err != ~0ull) {
        const std::string r = std::to_string((unsigned long long)(P.ust[i].err >> 8)), ci = n > 1 ? " (contig " + std::to_string(i) + " of the batch)" : std::string();
        switch ((uint32_t)(P.ust[i].err & 0xff)) {
            case fl::UP_PACKED:        return fail(FLORIA_E_INVALID, "packed pileup: the presence bits of read " + r + " do not match its first / last / cell count" + ci);
            case fl::UP_NO_CELLS:      return fail(FLORIA_E_INVALID, "read " + r + " has no cells (or read_off is not monotone)" + ci);
            case fl::UP_FIRST_LAST:    return fail(FLORIA_E_INVALID, "first/last of read " + r + " do not match its cells" + ci);
            case fl::UP_ONE_BASED:     return fail(FLORIA_E_INVALID, "SNP positions are 1-based" + ci);
            case fl::UP_NOT_ASCENDING: return fail(FLORIA_E_INVALID, "cells of read " + r + " not strictly ascending" + ci);
            case fl::UP_ALLELE:        return fail(FLORIA_E_UNSUPPORTED, "allele index > 3 (read " + r + ")" + ci);
            default:                   return fail(FLORIA_E_INVALID, "reads not sorted by Frag::cmp at read " + r + ci);
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        floria_hip_contig* c = new floria_hip_contig();
        c->ctx = ctx; c->arena = P.A; c->idx = i; c->n_reads = P.ucd[i].n_reads; c->n_cells = P.cp[i + 1] - P.cp[i];
        c->max_len = P.ust[i].max_len; c->n_alleles = P.ust[i].max_allele >= 2 ? 4 : 2; c->has_q0 = P.ust[i].has_q0 != 0;
        c->dev = dev(i);
        if (P.ust[i].no_pk) c->dev.cell_pk = nullptr;      // (a read spanning 2^20 SNP indices: no block can hold it, but nothing may decode its packed cells either)
        c->seq_pos = P.sp_dev.empty() ? nullptr : P.sp_dev[i];
        out[i] = c;
    }
    A->refs = n;
    A = nullptr;
    return 0;
}

}  // namespace

extern "C" {

// Upload a batch of contigs: plan the arena, DMA the raw arrays (consecutive contigs whose arrays are back to back in host
// memory travel as one transfer), validate + flatten on the device (upload_kernel.h), read back the per-contig status.
static int upload_batch_impl(floria_hip_ctx* ctx, const floria_pileup* pileups, const floria_pileup_packed* pk, uint32_t n, floria_hip_contig** out) {
    if (!ctx || !out || (n && !pileups && !pk)) return fail(FLORIA_E_INVALID, "null argument");
    for (uint32_t i = 0; i < n; ++i) out[i] = nullptr;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    EventTimer Tm(ctx->stream);                         // (before the plan: the plan's destructor waits for the device, the timer's events go after that)
    UploadPlan P;
    if (int rc = plan_upload(ctx, pileups, pk, n, 1, out, P)) return rc;
    const int th = Tm.begin(K_H2D);
    uint64_t pinned_b = 0, staged_b = 0;
    std::vector<CopyRun> runs = P.small_runs;
    runs.insert(runs.end(), P.chunk_runs[0].begin(), P.chunk_runs[0].end());
    if (int rc = issue_copies(ctx, runs, &pinned_b, &staged_b)) return rc;
    HIPCHK_AS("contig upload: ", issue_tables(ctx, P, ctx->stream));
    Tm.end(th);
    const int tk = Tm.begin(K_SEL);
    HIPCHK_AS("contig upload: ", launch_flatten(ctx, P, 0, ctx->stream));
    Tm.end(tk);
    HIPCHK_AS("contig upload: ", hipMemcpyAsync(P.ust.data(), P.T + P.t_st, sizeof(fl::UploadStatus) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK_AS("contig upload: ", hipStreamSynchronize(ctx->stream));
    if (int rc = P.commit()) return rc;
    ctx->timing = floria_timing{};
    Tm.publish(ctx->timing);
    ctx->timing.upload_pinned_bytes = pinned_b; ctx->timing.upload_staged_bytes = staged_b;
    return 0;
}
int floria_hip_contig_upload_batch(floria_hip_ctx* ctx, const floria_pileup* pileups, uint32_t n, floria_hip_contig** out) {
    return upload_batch_impl(ctx, pileups, nullptr, n, out);
}
int floria_hip_contig_upload_batch_packed(floria_hip_ctx* ctx, const floria_pileup_packed* pileups, uint32_t n, floria_hip_contig** out) {
    return upload_batch_impl(ctx, nullptr, pileups, n, out);
}

// The compact wire form of CSR pileups (include/floria_hip.h: floria_pileup_packed), host side.  A batch is laid out FIELD BY FIELD (every
// contig's read_off, then every bit_off, ...) at exactly the per-contig offsets plan_upload gives the device copies, so that an upload of the whole
// batch is one transfer per field (and per chunk) instead of seven per contig.
namespace {
struct PackLayout { std::vector<uint64_t> rp, cp, pb; size_t o_ro, o_bo, o_fi, o_la, o_pr, o_a2, o_qu, total; };
bool pack_layout(const floria_pileup* in, uint32_t n, PackLayout& Y) {
    Y.rp.assign(n + 1, 0); Y.cp.assign(n + 1, 0); Y.pb.assign(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const floria_pileup* p = &in[i];
        const uint64_t R = p->n_reads;
        if (R && (!p->read_off || !p->first || !p->last || !p->snp || !p->allele || !p->qual)) return false;
        uint64_t bits = 0;
        // read_off sizes every buffer (through read_off[R]) AND bounds the packing loop below, which runs before any device-side validation: it must be a
        // CSR offset array — 0 first, strictly ascending (a read without cells is refused by the CSR upload as well)
        if (R && p->read_off[0] != 0) return false;
        for (uint64_t r = 0; r < R; ++r) {
            if (p->last[r] < p->first[r] || p->read_off[r + 1] <= p->read_off[r]) return false;
            bits += (uint64_t)p->last[r] - p->first[r] + 1;
        }
        if (bits >= (1ull << 32)) return false;
        Y.rp[i + 1] = Y.rp[i] + R; Y.cp[i + 1] = Y.cp[i] + (R ? p->read_off[R] : 0); Y.pb[i + 1] = Y.pb[i] + (bits + 7) / 8 + 1;
    }
    size_t cur = 0;
    auto seg = [&](uint64_t bytes) { const size_t o = cur; cur += (size_t)((bytes + 63) & ~(uint64_t)63); return o; };
    const uint64_t R = Y.rp[n], C = Y.cp[n];
    Y.o_ro = seg(4 * (R + n)); Y.o_bo = seg(4 * (R + n)); Y.o_fi = seg(4 * R); Y.o_la = seg(4 * R);
    Y.o_pr = seg(Y.pb[n] + 16); Y.o_a2 = seg(C / 4 + n + 16); Y.o_qu = seg(C + 16);
    Y.total = cur;
    return true;
}
}  // namespace
size_t floria_hip_pack_bytes_batch(const floria_pileup* in, uint32_t n) {
    PackLayout Y;
    if (!in || !n || !pack_layout(in, n, Y)) return 0;
    return Y.total;
}
int floria_hip_pack_pileups_batch(const floria_pileup* in, uint32_t n, void* buf, size_t buf_bytes, floria_pileup_packed* out) {
    if ((n && (!in || !out)) || (!buf && buf_bytes)) return fail(FLORIA_E_INVALID, "null argument");
    if (!n) return 0;
    PackLayout Y;
    if (!pack_layout(in, n, Y)) return fail(FLORIA_E_INVALID, "pileup cannot be packed (null field, read_off not a strictly ascending offset array from 0, last < first, or spans of 2^32 bits and more)");
    if (buf_bytes < Y.total) return fail(FLORIA_E_INVALID, "pack buffer too small (floria_hip_pack_bytes_batch)");
    char* B = (char*)buf;
    memset(B + Y.o_pr, 0, Y.pb[n] + 16); memset(B + Y.o_a2, 0, Y.cp[n] / 4 + n + 16);
    for (uint32_t i = 0; i < n; ++i) {
        const floria_pileup* p = &in[i];
        const uint64_t R = p->n_reads, C = R ? p->read_off[R] : 0;
        uint32_t* ro = (uint32_t*)(B + Y.o_ro + 4 * (Y.rp[i] + i)); uint32_t* bo = (uint32_t*)(B + Y.o_bo + 4 * (Y.rp[i] + i));
        uint32_t* fi = (uint32_t*)(B + Y.o_fi + 4 * Y.rp[i]);       uint32_t* la = (uint32_t*)(B + Y.o_la + 4 * Y.rp[i]);
        uint8_t* pr = (uint8_t*)(B + Y.o_pr + Y.pb[i]); uint8_t* a2 = (uint8_t*)(B + Y.o_a2 + Y.cp[i] / 4 + i); uint8_t* qu = (uint8_t*)(B + Y.o_qu + Y.cp[i]);
        uint64_t bit = 0;
        for (uint64_t r = 0; r < R; ++r) {
            ro[r] = p->read_off[r]; fi[r] = p->first[r]; la[r] = p->last[r]; bo[r] = (uint32_t)bit;
            const uint32_t F = p->first[r], span = p->last[r] - F + 1;
            for (uint32_t c = p->read_off[r]; c < p->read_off[r + 1]; ++c) {
                const uint32_t sp = p->snp[c];
                if (sp < F || sp - F >= span || p->allele[c] > 3) {
                    const std::string where = " (read " + std::to_string((unsigned long long)r) + (n > 1 ? ", contig " + std::to_string(i) + " of the batch)" : ")");
                    if (p->allele[c] > 3 && !(sp < F || sp - F >= span)) return fail(FLORIA_E_UNSUPPORTED, "allele index > 3" + where);
                    return fail(FLORIA_E_INVALID, "cell outside [first, last]" + where);
                }
                const uint64_t bi = bit + (sp - F);
                pr[bi >> 3] |= (uint8_t)(1u << (bi & 7));
                a2[c >> 2] |= (uint8_t)(p->allele[c] << (2 * (c & 3)));
            }
            bit += span;
        }
        ro[R] = (uint32_t)C; bo[R] = (uint32_t)bit;
        if (C) memcpy(qu, p->qual, C);
        out[i] = floria_pileup_packed{ro, fi, la, bo, pr, a2, qu, p->n_reads, p->set_order};      // (the optional set order is not repacked: the packed pileup points at the caller's array)
    }
    return 0;
}
size_t floria_hip_pack_bytes(const floria_pileup* in) { return floria_hip_pack_bytes_batch(in, in ? 1 : 0); }
int floria_hip_pack_pileup(const floria_pileup* in, void* buf, size_t buf_bytes, floria_pileup_packed* out) {
    if (!in || !out) return fail(FLORIA_E_INVALID, "null argument");
    return floria_hip_pack_pileups_batch(in, 1, buf, buf_bytes, out);
}



int floria_hip_contig_upload(floria_hip_ctx* ctx, const floria_pileup* p, floria_hip_contig** out) {
    if (!ctx || !out || !p) return fail(FLORIA_E_INVALID, p ? "null argument" : "null pileup");
    return floria_hip_contig_upload_batch(ctx, p, 1, out);
}
void floria_hip_contig_free(floria_hip_contig* c) {
    if (!c) return;
    if (c->arena && --c->arena->refs == 0) arena_put(c->arena);
    delete c;
}

// Diagnostic: copy one resident array of a contig back to the host (tests compare the device-side flatten with the formulas).
int floria_hip_contig_download(const floria_hip_contig* c, int field, void* dst, size_t bytes) {
    if (!c || (!dst && bytes)) return fail(FLORIA_E_INVALID, "null argument");
    const void* src = nullptr;
    size_t have = 0;
    switch (field) {
        case FLORIA_FIELD_READ_OFF: src = c->dev.read_off; have = 4ull * (c->n_reads + (c->n_reads ? 1 : 0)); break;
        case FLORIA_FIELD_FIRST:    src = c->dev.first;    have = 4ull * c->n_reads; break;
        case FLORIA_FIELD_LAST:     src = c->dev.last;     have = 4ull * c->n_reads; break;
        case FLORIA_FIELD_SNP:      src = c->dev.cell_snp; have = 4ull * c->n_cells; break;
        case FLORIA_FIELD_CELL_AW:  src = c->dev.cell_aw;  have = 4ull * c->n_cells; break;
        case FLORIA_FIELD_TW:       src = c->dev.tw;       have = 16ull * c->n_reads; break;
        case FLORIA_FIELD_META:     src = c->dev.meta;     have = 32ull * c->n_reads; break;
        case FLORIA_FIELD_SET_ORDER:
            if (!c->dev.set_order) return fail(FLORIA_E_INVALID, "the contig carries no set_order");
            src = c->dev.set_order; have = 4ull * c->n_cells; break;
        case FLORIA_FIELD_SEQ_POS:
            // (to a contig without positions the field stays what it was before positions existed, an unknown field, and the message keeps saying so)
            if (!c->seq_pos) return fail(FLORIA_E_INVALID, "the contig carries no seq_pos (field 8 is an unknown field of a contig without positions)");
            src = c->seq_pos; have = 4ull * c->n_cells; break;
        default: return fail(FLORIA_E_INVALID, "unknown field");
    }
    if (bytes > have) return fail(FLORIA_E_INVALID, "field is smaller than the requested size");
    HIPCHK(hipSetDevice(c->ctx->device));
    if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

namespace {

Arena* arena_get(floria_hip_ctx* ctx, size_t bytes) {
    Arena* a = nullptr;
    // best fit among the cached arenas, else grow the largest, else a new one
    size_t best = (size_t)-1;
    for (size_t i = 0; i < ctx->arena_cache.size(); ++i) if (ctx->arena_cache[i]->buf.cap >= bytes && (best == (size_t)-1 || ctx->arena_cache[i]->buf.cap < ctx->arena_cache[best]->buf.cap)) best = i;
    if (best == (size_t)-1 && !ctx->arena_cache.empty()) { best = 0; for (size_t i = 1; i < ctx->arena_cache.size(); ++i) if (ctx->arena_cache[i]->buf.cap > ctx->arena_cache[best]->buf.cap) best = i; }
    if (best != (size_t)-1) { a = ctx->arena_cache[best]; ctx->arena_cache.erase(ctx->arena_cache.begin() + best); }
    else { a = new Arena(); a->ctx = ctx; }
    if (a->buf.ensure(bytes)) { a->buf.release(); delete a; return nullptr; }
    a->refs = 0; a->host_meta = false;
    return a;
}
void arena_put(Arena* a) {
    floria_hip_ctx* ctx = a->ctx;
    a->h_first.clear(); a->h_last.clear(); a->host_meta = false; a->refs = 0;
    if (ctx->arena_cache.size() < 4) ctx->arena_cache.push_back(a);
    else { a->buf.release(); delete a; }
}

int issue_copies(floria_hip_ctx* ctx, std::vector<CopyRun>& runs, uint64_t* pinned_bytes, uint64_t* staged_bytes) {
    std::vector<CopyRun> staged;          // pageable runs, cut into SEG pieces
    for (const CopyRun& r : runs) {
        const bool pin = r.bytes >= 4096 && is_pinned(r.src) && is_pinned(r.src + r.bytes - 1);
        if (pin) {
            *pinned_bytes += r.bytes;
            HIPCHK(hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            *staged_bytes += r.bytes;
            for (size_t o = 0; o < r.bytes; o += StagePool::SEG) staged.push_back({r.src + o, r.dst + o, std::min(StagePool::SEG, r.bytes - o)});
        }
    }
    if (staged.empty()) return 0;
    size_t tot = 0;
    for (auto& r : staged) tot += r.bytes;
    if (tot < (1u << 20)) {                  // small: let the runtime stage it
        for (auto& r : staged) HIPCHK(hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    if (int rc = ctx->stage.init()) return rc;
    StagePool& SP = ctx->stage;
    if (!ctx->copy_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->ev_rids) HIPCHK(hipEventCreateWithFlags(&ctx->ev_rids, hipEventDisableTiming));
    // Worker threads only memcpy (pageable source -> pinned segment); THIS thread makes every HIP call: it issues the DMA of
    // segment k as soon as it is filled — alternating between two streams, so the completion latency of one copy hides behind
    // the next — and hands a staging buffer back to the fillers once the DMA that read it has completed.
    const uint32_t nseg = (uint32_t)staged.size();
    const uint32_t nthreads = std::max(1u, std::min<uint32_t>({ctx->stage_threads, nseg, 16u}));
    std::vector<std::atomic<int>> filled(nseg);
    for (auto& f : filled) f.store(0);
    std::atomic<uint32_t> next{0}, freed{StagePool::NBUF};     // segments < freed may be filled (their buffer is free)
    std::atomic<int> failed{0};
    auto worker = [&]() {
        for (;;) {
            const uint32_t k = next.fetch_add(1);
            if (k >= nseg) return;
            while (freed.load(std::memory_order_acquire) <= k) { if (failed.load()) return; std::this_thread::yield(); }
            memcpy(SP.buf[k % StagePool::NBUF], staged[k].src, staged[k].bytes);
            filled[k].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(worker);
    hipStream_t cs[2] = {ctx->stream, ctx->copy_stream};
    hipError_t e = hipEventRecord(ctx->ev_rids, ctx->stream);                       // the second stream starts after what the first has queued
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, ctx->ev_rids, 0);
    uint32_t done = 0;                                                              // DMAs known complete
    for (uint32_t k = 0; k < nseg && e == hipSuccess; ++k) {
        while (!filled[k].load(std::memory_order_acquire)) {
            // while waiting for the fillers, retire completed DMAs so that their buffers can be refilled
            if (done < k && hipEventQuery(SP.ev[done % StagePool::NBUF]) == hipSuccess) { ++done; freed.store(done + StagePool::NBUF, std::memory_order_release); }
            else std::this_thread::yield();
        }
        e = hipMemcpyAsync(staged[k].dst, SP.buf[k % StagePool::NBUF], staged[k].bytes, hipMemcpyHostToDevice, cs[k & 1]);
        if (e == hipSuccess) e = hipEventRecord(SP.ev[k % StagePool::NBUF], cs[k & 1]);
        // the fillers may be blocked on a buffer whose DMA is still running: wait for the oldest one when the ring is exhausted
        while (e == hipSuccess && done + StagePool::NBUF <= k + 1 && k + 1 < nseg && freed.load() <= k + 1) {
            e = hipEventSynchronize(SP.ev[done % StagePool::NBUF]);
            ++done; freed.store(done + StagePool::NBUF, std::memory_order_release);
        }
    }
    if (e != hipSuccess) failed.store(1);
    freed.store(0xffffffffu);
    for (auto& t : th) t.join();
    (void)hipGetLastError();                                                        // hipEventQuery's hipErrorNotReady is not an error
    if (e == hipSuccess) e = hipEventRecord(ctx->ev_rids, ctx->copy_stream);        // the main stream continues after both
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_rids, 0);
    if (e != hipSuccess) { sync_all(ctx); return fail(FLORIA_E_DEVICE, std::string("staged upload failed: ") + hipGetErrorString(e)); }
    return 0;
}

}  // namespace

extern "C" {

// ---- S1 --------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// Reference-arithmetic mode: the cells of every read of the given contigs in the iteration order of its position set (cell_order_kernel), for
// the call in flight: ctx->cur_ord[ctx->cur_ord_off[c] + read_off[r] + x] = {SNP, allele << 28 | weight} of the x-th position of read r's set.
// Computed by two launches (round 5: ≈ 130 ms for the 331 M cells of config 4 with the one-thread-per-read table emulation alone) and kept until the context uploads contigs again: S2 after S1, or the next S1 call over the same resident batch, reuses it.
struct OrderPlan {                        // host side of the cell orders of one set of contigs
    std::vector<uint64_t> pre;            // reads before contig c [n+1] | cells before contig c [n] | [1 pad] | status word of the host-given set orders
    uint64_t cells = 0, R_all = 0, sig = 0;
    uint32_t n_contigs = 0;
};
void order_plan(const std::vector<fl::ContigDev>& cdev, const std::vector<uint64_t>& n_cells, OrderPlan& O) {
    const uint32_t n_contigs = O.n_contigs = (uint32_t)cdev.size();
    O.pre.assign(2 * (size_t)n_contigs + 3, 0);
    uint64_t cells = 0;
    for (uint32_t i = 0; i < n_contigs; ++i) { O.pre[i + 1] = O.pre[i] + cdev[i].n_reads; O.pre[n_contigs + 1 + i] = cells; cells += n_cells[i]; }
    O.cells = cells; O.R_all = O.pre[n_contigs];
    uint64_t sig = 1469598103934665603ull;                                    // FNV-1a over what identifies the contigs: their device arrays and sizes
    auto mix = [&](uint64_t v) { for (int b = 0; b < 8; ++b) { sig ^= (v >> (8 * b)) & 0xff; sig *= 1099511628211ull; } };
    for (uint32_t i = 0; i < n_contigs; ++i) { mix((uint64_t)(uintptr_t)cdev[i].cell_snp); mix((uint64_t)(uintptr_t)cdev[i].read_off); mix(cdev[i].n_reads); mix(n_cells[i]); mix((uint64_t)(uintptr_t)cdev[i].set_order); }
    O.sig = sig;
}
// the two launches for the reads [r0, r1) of the contigs [c0, c1) on `st` (their cells must have been flattened on that stream, or before it)
int order_launch(floria_hip_ctx* ctx, const OrderPlan& O, const fl::ContigDev* d_contigs, uint32_t c0, uint32_t c1, uint64_t* todo, uint8_t* scratch, uint64_t scratch_bytes, uint32_t len_max,
                 const uint32_t* status_max_len, hipStream_t st) {
    const uint64_t r0 = O.pre[c0], nr = O.pre[c1] - r0;
    if (!nr) return 0;
    fl::CellOrderArgs oa{};
    oa.todo = todo; oa.replay_all = ctx->knobs.arith_replay;
    oa.bad = ctx->arith_tab.as<uint64_t>() + 2 * (size_t)O.n_contigs + 2;
    oa.contigs = d_contigs + c0; oa.read_prefix = ctx->arith_tab.as<uint64_t>() + c0; oa.cell_prefix = ctx->arith_tab.as<uint64_t>() + O.n_contigs + 1 + c0;
    oa.n_contigs = c1 - c0; oa.n_reads = nr; oa.read_base = r0; oa.ord = ctx->arith_ord.as<uint2>(); oa.scratch = scratch; oa.scratch_bytes = scratch_bytes;
    oa.len_max = len_max; oa.status_max_len = status_max_len; oa.status_stride = (uint32_t)(sizeof(fl::UploadStatus) / 4);
    uint64_t nth = std::min<uint64_t>((nr + 255) & ~255ull, 131072);
    if (len_max) {
        oa.ctrl_bytes = fl::fx_ctrl_bytes(len_max); oa.slot_bytes = fl::fx_slot_bytes(len_max);
        nth = std::max<uint64_t>(256, std::min<uint64_t>(nth, (scratch_bytes / (3 * (oa.ctrl_bytes + oa.slot_bytes))) & ~255ull));
    } else nth = std::min<uint64_t>(nth, 16384);
    // a wavefront per read where the home-bucket rule applies or the host gave the order (arith_kernel.h), then one thread per read for the rest (none on BASELINE's configs)
    hipLaunchKernelGGL(fl::cell_order_direct_kernel, dim3((uint32_t)std::min<uint64_t>((nr + 3) / 4, (uint64_t)ctx->n_cu * 16)), dim3(256), 0, st, oa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fl::cell_order_kernel, dim3((uint32_t)(nth / 256)), dim3(256), 0, st, oa);
    HIPCHK(hipGetLastError());
    return 0;
}
int order_bad_read(const OrderPlan& O, uint64_t bad) {
    if (!bad) return 0;
    uint32_t ci = 0;
    const uint64_t gr = ~bad;
    while (ci + 1 < O.n_contigs && O.pre[ci + 1] <= gr) ++ci;
    return fail(FLORIA_E_INVALID, "set_order of read " + std::to_string((unsigned long long)(gr - O.pre[ci])) + (O.n_contigs > 1 ? " (contig " + std::to_string(ci) + " of the batch)" : std::string())
                                  + " is not a permutation of the indices of its cells");
}
int cell_orders(floria_hip_ctx* ctx, const fl::ContigDev* d_contigs, const std::vector<fl::ContigDev>& cdev, const std::vector<uint64_t>& n_cells, uint32_t len_max) {
    const uint32_t n_contigs = (uint32_t)cdev.size();
    OrderPlan O;
    order_plan(cdev, n_cells, O);
    if (ctx->ord_epoch == ctx->upload_epoch && ctx->ord_sig == O.sig && ctx->arith_ord.p && ctx->arith_tab.p) {
        ctx->cur_ord = ctx->arith_ord.as<uint2>(); ctx->cur_ord_off = ctx->arith_tab.as<uint64_t>() + n_contigs + 1;
        return 0;
    }
    int rc = ctx->arith_tab.ensure(O.pre.size() * 8); if (rc) return rc;
    rc = ctx->arith_ord.ensure(8 * O.cells + 16); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->arith_tab.p, O.pre.data(), O.pre.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                                // (`pre` is pageable and local)
    if (O.R_all) {
        const uint64_t tb = fl::fx_ctrl_bytes(std::max(1u, len_max)) + fl::fx_slot_bytes(std::max(1u, len_max));
        uint64_t nth = std::min<uint64_t>((O.R_all + 255) & ~255ull, 131072);
        nth = std::max<uint64_t>(256, std::min<uint64_t>(nth, ((2ull << 30) / (3 * tb)) & ~255ull));
        const uint64_t todo_bytes = (8 * (O.R_all + 1) + 255) & ~255ull;          // [count | reads for the table emulation] in front of the emulation's scratch
        rc = ctx->arith_scr.ensure(todo_bytes + 3 * tb * nth); if (rc) return rc;
        HIPCHK(hipMemsetAsync(ctx->arith_scr.p, 0, 8, ctx->stream));
        rc = order_launch(ctx, O, d_contigs, 0, n_contigs, ctx->arith_scr.as<uint64_t>(), ctx->arith_scr.as<uint8_t>() + todo_bytes, 3 * tb * nth, std::max(1u, len_max), nullptr, ctx->stream);
        if (rc) return rc;
        bool any_given = false;
        for (uint32_t i = 0; i < n_contigs; ++i) any_given = any_given || cdev[i].set_order != nullptr;
        if (any_given) {                                                       // a host-given order that is not a permutation of a read's cells: refuse the call
            uint64_t bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, ctx->arith_tab.as<uint64_t>() + 2 * (size_t)n_contigs + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (int brc = order_bad_read(O, bad)) return brc;
        }
    }
    ctx->cur_ord = ctx->arith_ord.as<uint2>(); ctx->cur_ord_off = ctx->arith_tab.as<uint64_t>() + n_contigs + 1;
    ctx->ord_epoch = ctx->upload_epoch; ctx->ord_sig = O.sig;
    return 0;
}

// What S1 needs to know about its contigs.  With `chunk_ev` the cell arrays of chunk g (contig_chunk[ci] == g) are still on
// the wire: they are complete once chunk_ev[g] has fired, and the blocks of chunk g form job group g whose stream waits for it
// (read_off / first / last of every contig are already ordered before the context's main stream).
struct S1Contigs {
    std::vector<fl::ContigDev> cdev;
    std::vector<uint64_t> n_cells;     // per contig (reference-arithmetic mode: the layout of the cell orders)
    uint32_t len_max = 1, nall = 2;
    bool any_q0 = false;
    const uint32_t* contig_chunk = nullptr;
    uint32_t n_chunks = 0;
    hipEvent_t* chunk_ev = nullptr;
    bool orders_in_flight = false; // reference-arithmetic mode, pipelined upload: every chunk's cell orders are computed behind its flatten launch, ahead of its event
    uint32_t chunk_groups = 0;     // job groups the chunks are merged into (0 = one per chunk)
    bool ends_apart = false;       // with three groups: first chunk | middle chunks | last chunk
};

// host mailbox -> device array, by a kernel on the call's own stream (no copy engine involved)
__global__ void box_copy_kernel(uint32_t* dst, const uint32_t* src, uint32_t n_words) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

struct Trace {
    bool on; std::chrono::steady_clock::time_point t0;
    explicit Trace(bool o) : on(o), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what) const { if (on) fprintf(stderr, "[floria_hip trace] %8.3f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what); }
};

// job groups (longest-first inside each group).  Resident inputs: dealt round-robin so every group sees the same size mix.
// Chunked inputs (cells still arriving): group g = the blocks of chunk g, whose stream waits for the chunk's event (group_ev[g]).
// Reorders jobs (longest first) group after group and returns where each group starts (G + 1 offsets).
std::vector<uint32_t> job_groups(const floria_hip_ctx* ctx, const S1Contigs& SC, bool chunked, const std::vector<uint32_t>& bc, std::vector<uint32_t>& jobs,
                                 hipEvent_t* group_ev) {
    // (measured, config 4, resident: one group wins while a stage has less than three rounds of jobs — 750 / 1000 / 1500 contigs: 55 / 61.5 / 80.5 ms against
    // 58.7 / 68 / 82 ms with two groups — two groups win from there: 2000 contigs 96.4 against 99.4 ms.  End of round 4 (profiles/r04_groups_ab.txt), ms per
    // step with 1 / 2 / 3 / 4 groups: 7 249 blocks 51.6 / 55.2 / 51.4 / -, 10 875 blocks 67.8 / 66.7 / 65.3 / -, 14 503 blocks 81.6 / 78.8 / 75.9 or 79.3 / 78.4-79.1:
    // three groups are 3.7 % faster in five runs of seven and level in the other two (the three chains interleave in one of two patterns); the pipelined call,
    // which has its own three chunk groups, does not change.  Round 5 (profiles/r05_groups_ab.txt; box A, three interleaved runs): 2 groups 79.5 / 79.6 / 80.2,
    // 3 groups 77.3 / 76.1 / 77.2, 4 groups with half-size grids 78.9 / 79.3 / 79.2, an equal share of the wave slots per group (3 x 1 366) 81.8-82.2; box B, in the
    // default bench flow and resident-only: 2 groups 79.9-80.3 (six runs), 3 groups 80.3 / 80.7 / 79.8 / 79.8 / 77.5 / 78.3; 1500 contigs 64.5 against 67.8 (2) and
    // 68.6 (1).  Three groups land on the level of two or 3 % below it, never above by more than the noise -> three from 40 x CUs blocks on (round 4 kept two for
    // the per-launch roofline fraction, which is not what a step costs).  Unequal groups (dealing weights 10:8:6 .. 14:8:2) do not pin the good pattern (78.4-80.9).
    uint32_t G = ctx->knobs.groups ? ctx->knobs.groups : (jobs.size() >= (size_t)ctx->n_cu * 40 ? 3 : 1);
    G = std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(G, floria_hip_ctx::MAX_GROUPS), (uint32_t)(jobs.size() / 1024)));
    if (ctx->hw_queues < 5 && !ctx->knobs.groups) G = std::min<uint32_t>(G, 2);
    // chunked: consecutive chunks may share a job group (SC.chunk_groups), which then starts when its LAST chunk has landed
    std::vector<uint32_t> chunk_group;
    if (chunked) {
        const uint32_t nc = std::min<uint32_t>(SC.n_chunks, floria_hip_ctx::MAX_GROUPS);
        G = SC.chunk_groups ? std::min<uint32_t>(SC.chunk_groups, nc) : nc;
        if (ctx->hw_queues < 5) G = std::min<uint32_t>(G, 2);          // (groups on shared hardware queues serialise: two at most)
        chunk_group.resize(SC.n_chunks);
        for (uint32_t c = 0; c < SC.n_chunks; ++c) {
            const uint32_t cc = std::min(c, nc - 1);
            // ends_apart: the first chunk is a group of its own (it starts while the rest is still arriving and is too small to own every wave slot), so is the last
            chunk_group[c] = SC.ends_apart && G == 3 && nc >= 3 ? (cc == 0 ? 0u : cc == nc - 1 ? 2u : 1u) : std::min<uint32_t>((uint32_t)((uint64_t)cc * G / nc), G - 1);
            group_ev[chunk_group[c]] = SC.chunk_ev[cc];
        }
    }
    std::vector<uint32_t> group_off(G + 1, 0);
    if (chunked) {
        std::vector<uint32_t> dealt; dealt.reserve(jobs.size());
        for (uint32_t g = 0; g < G; ++g) { for (uint32_t b : jobs) if (chunk_group[SC.contig_chunk[bc[b]]] == g) dealt.push_back(b); group_off[g + 1] = (uint32_t)dealt.size(); }
        jobs.swap(dealt);
    } else if (G > 1) {
        std::vector<uint32_t> dealt; dealt.reserve(jobs.size());
        for (uint32_t g = 0; g < G; ++g) { for (size_t j = g; j < jobs.size(); j += G) dealt.push_back(jobs[j]); group_off[g + 1] = (uint32_t)dealt.size(); }
        jobs.swap(dealt);
    } else group_off[1] = (uint32_t)jobs.size();
    return group_off;
}

// ploidy stages (run_phase): one ploidy per stage unless the batch is too small to fill the chip with (block, ploidy) jobs
std::vector<std::vector<uint32_t>> ploidy_stages(const floria_hip_ctx* ctx, const floria_params* prm, size_t n_jobs, uint32_t G) {
    const uint32_t P = prm->max_ploidy;
    std::vector<std::vector<uint32_t>> stages;
    int spec = ctx->knobs.speculate;
    const bool slab_path = P * prm->beam <= 63 && !ctx->knobs.beam_path;          // the wide-beam kernels own whole CUs: nothing to gain there
    // (measured on config-4 shards, resident, with the gated high ploidies and the early stop-rule flags of run_phase; ms for speculate = 0 / 1 / 2:
    //   915 blocks 37.6 / 21.3 / 24.3   1822: 40.4 / 24.8 / 27.1   2724: 44.1 / 32.2 / 32.7   3636: 48.0 / 46.5 / 36.8   4543: 50.9 / 57.7 / 44.9
    //   5455: 55.5 / 69.1 / 50.9   6348: 58.7 / 80.8 / 56.9   7249: 61.6 / - / 62.5   14503: 98.6 / 141-155 / 115.5)
    // round 4, faster beam steps (scripts/shard_sweep.py, profiles/r04_shard_sweep.txt; ms for speculate = 0 / 1 / 2):
    //   915: 32.7 / 19.8 / 26.6   1822: 36.1 / 23.0 / 29.5   2724: 40.6 / 31.3 / 34.9   3636: 43.2 / 36.1 / 39.5   4543: 46.6 / 42.2 / 44.2
    //   5455: 50.4 / 50.3 / 48.9   6348: 52.7 / 56.0 / 53.3   7249: 56.8 / 63.7 / 58.1
    // -> every ploidy at once up to 18 x CUs blocks, {1,2,3} then {4..P} up to 23 x CUs, one ploidy per stage above
    if (spec < 0) spec = !(slab_path && P >= 3) ? 0 : n_jobs <= (size_t)ctx->n_cu * 18 ? 1 : (n_jobs <= (size_t)ctx->n_cu * 23 && P >= 4) ? 2 : 0;
    if (P * G > floria_hip_ctx::MAX_LANES || P < 3) spec = 0;
    // a speculative stage's lanes wait on each other's events: with more lanes than hardware queues (GPU_MAX_HW_QUEUES, 12 in our hosts, minus the main,
    // copy and flatten streams) they share queues and the gates serialise the stage (measured: 250 contigs in 3 / 4 / 5 chunk groups 94 / 141 / 187 ms against 32)
    // (floria_hip_create measured how many streams really run side by side: hw_queues; main, copy and flatten streams take up to three of them)
    // With GPU_MAX_HW_QUEUES=12 the probe sees 6 spinning kernels side by side on an MI355X, and stages of up to 10 lanes measured fine (round 2: 250
    // contigs 24-26 ms against 38 without); with the runtime's default of 4 queues it sees 4 or fewer, and there the gated lanes serialise (3-8x).
    const uint32_t lanes_ok = ctx->hw_queues >= 5 ? 10u : (ctx->hw_queues > 1 ? ctx->hw_queues - 1 : 1u);
    if (ctx->knobs.speculate < 0 && spec) { const uint32_t w = spec == 1 ? P : std::max<uint32_t>(std::min(3u, P), P > 3 ? P - 3 : 0); if (w * G > lanes_ok) spec = 0; }
    if (spec == 3 && P >= 5) {          // {1}{2}{3}{4..P}: only the ploidies few blocks reach run side by side
        for (uint32_t p = 1; p <= 3; ++p) stages.push_back({p});
        stages.emplace_back(); for (uint32_t p = 4; p <= P; ++p) stages.back().push_back(p);
    }
    else if (spec == 1) { stages.emplace_back(); for (uint32_t p = 1; p <= P; ++p) stages.back().push_back(p); }
    else if (spec == 2) { stages.emplace_back(); for (uint32_t p = 1; p <= std::min(3u, P); ++p) stages.back().push_back(p);
                          if (P > 3) { stages.emplace_back(); for (uint32_t p = 4; p <= P; ++p) stages.back().push_back(p); } }
    else for (uint32_t p = 1; p <= P; ++p) stages.push_back({p});
    if (spec == 3 && P < 5) { stages.clear(); for (uint32_t p = 1; p <= P; ++p) stages.push_back({p}); }
    // one ploidy per stage: ploidy 1 needs no stage of its own where the ploidy-2 optimise job computes it on the way (Knobs::fuse_p1; run_phase sees that no stage holds ploidy 1)
    const Knobs& K = ctx->knobs;
    if (stages.size() == P && P >= 2 && !K.arith && !K.no_p1_shortcut && K.fuse_p1 != 0) stages.erase(stages.begin());
    return stages;
}

int s1_core(floria_hip_ctx* ctx, const S1Contigs& SC, const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end,
            uint32_t n_blocks, const floria_params* prm, floria_block_result** out) {
    const uint32_t n_contigs = (uint32_t)SC.cdev.size();
    const Trace TR(ctx->knobs.trace);
    TR.mark("s1_core enter");
    if (prm->max_ploidy < 1 || prm->max_ploidy > FLORIA_MAX_PLOIDY) return fail(FLORIA_E_INVALID, "max_ploidy must be in 1..16");
    if (prm->beam < 1) return fail(FLORIA_E_INVALID, "beam (max_number_solns) must be >= 1");
    if (!(prm->epsilon > 0.0 && prm->epsilon < 1.0)) return fail(FLORIA_E_INVALID, "epsilon must be in (0,1)");
    ctx->timing = floria_timing{};
    ctx->batch_token = 0; ctx->last_contigs.clear();
    const uint32_t P = prm->max_ploidy;

    // ---- block read lists: find_reads_in_interval on the device (blocks_kernel.h) -------------------------------
    std::vector<uint32_t> bc(n_blocks, 0);
    uint32_t n_max = 1, span_max = 1;
    const uint32_t len_max = SC.len_max, nall = SC.nall;
    const bool any_q0 = SC.any_q0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t ci = blk_contig ? blk_contig[b] : 0;
        if (ci >= n_contigs) return fail(FLORIA_E_INVALID, "blk_contig out of range");
        bc[b] = ci;
    }
    const std::vector<fl::ContigDev>& cdev = SC.cdev;
    Carve C0;
    const Seg s_cdev = C0.seg(sizeof(fl::ContigDev) * std::max(1u, n_contigs)), s_bc = C0.seg(4ull * n_blocks + 4), s_bs = C0.seg(4ull * n_blocks + 4),
              s_be = C0.seg(4ull * n_blocks + 4), s_p0 = C0.seg(4ull * n_blocks + 4), s_sp = C0.seg(4ull * n_blocks + 4), s_cnt = C0.seg(4ull * n_blocks + 4),
              s_bytes = C0.seg(8ull * n_blocks + 8), s_roff = C0.seg(8ull * (n_blocks + 1));
    int rc = C0.place(ctx->misc0); if (rc) return rc;
    EventTimer T(ctx->stream);
    // the call's small transfers go through the context's host mailbox (HostBox): up by a copy kernel on the main stream, down by the kernel's own stores
    static_assert(sizeof(fl::ContigDev) % 4 == 0, "box_copy_kernel moves 4-byte words");
    size_t box_cur = 0;
    auto box_take = [&](size_t bytes) { const size_t o = box_cur; box_cur += (bytes + 63) & ~(size_t)63; return o; };
    const size_t bx_cdev = box_take(sizeof(fl::ContigDev) * n_contigs), bx_bc = box_take(4ull * n_blocks), bx_bs = box_take(4ull * n_blocks), bx_be = box_take(4ull * n_blocks),
                 bx_cnt = box_take(4ull * n_blocks), bx_span = box_take(4ull * n_blocks), bx_bytes = box_take(8ull * n_blocks), bx_roff = box_take(8ull * (n_blocks + 1)),
                 bx_jobs = box_take(4ull * n_blocks);
    rc = ctx->box.ensure(box_cur + 64); if (rc) return rc;
    auto box_up = [&](void* dst, const void* src, size_t bytes, size_t at) -> hipError_t {
        if (!bytes) return hipSuccess;
        memcpy(ctx->box.h + at, src, bytes);
        const uint32_t words = (uint32_t)(bytes / 4);
        hipLaunchKernelGGL(box_copy_kernel, dim3(std::max(1u, std::min(256u, (words + 255) / 256))), dim3(256), 0, ctx->stream, (uint32_t*)dst, (const uint32_t*)(ctx->box.d + at), words);
        return hipGetLastError();
    };
    int th = T.begin(K_H2D);
    HIPCHK(box_up(C0.at(s_cdev), cdev.data(), sizeof(fl::ContigDev) * n_contigs, bx_cdev));
    if (n_blocks) {
        HIPCHK(box_up(C0.at(s_bc), bc.data(), 4ull * n_blocks, bx_bc));
        HIPCHK(box_up(C0.at(s_bs), blk_start, 4ull * n_blocks, bx_bs));
        HIPCHK(box_up(C0.at(s_be), blk_end, 4ull * n_blocks, bx_be));
    }
    T.end(th);
    fl::ScanArgs sa{};
    sa.contigs = C0.at<const fl::ContigDev>(s_cdev);
    sa.blk_contig = C0.at<const uint32_t>(s_bc); sa.blk_start = C0.at<const uint32_t>(s_bs); sa.blk_end = C0.at<const uint32_t>(s_be);
    sa.n_blocks = n_blocks; sa.max_ploidy = P;
    sa.cnt = C0.at<uint32_t>(s_cnt); sa.pos0 = C0.at<uint32_t>(s_p0); sa.span = C0.at<uint32_t>(s_sp); sa.bytes = C0.at<uint64_t>(s_bytes);
    sa.h_cnt = (uint32_t*)(ctx->box.d + bx_cnt); sa.h_span = (uint32_t*)(ctx->box.d + bx_span); sa.h_bytes = (uint64_t*)(ctx->box.d + bx_bytes);
    std::vector<uint32_t> cnt(n_blocks, 0), span(n_blocks, 0);
    std::vector<uint64_t> blk_bytes(n_blocks, 0), roff(n_blocks + 1, 0);
    if (n_blocks) {
        int tk = T.begin(K_SEL);
        hipLaunchKernelGGL(fl::block_reads_kernel<false>, dim3(n_blocks), dim3(64), 0, ctx->stream, sa);
        T.end(tk);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));           // (the kernel wrote its counts into the mailbox)
        memcpy(cnt.data(), ctx->box.h + bx_cnt, 4ull * n_blocks);
        memcpy(span.data(), ctx->box.h + bx_span, 4ull * n_blocks);
        memcpy(blk_bytes.data(), ctx->box.h + bx_bytes, 8ull * n_blocks);
    }
    TR.mark("block counts on the host");
    uint64_t algo_bytes = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        roff[b + 1] = roff[b] + cnt[b];
        n_max = std::max(n_max, cnt[b]); span_max = std::max(span_max, span[b]);
        algo_bytes += blk_bytes[b];
    }
    if (n_max >= (1u << 20)) return fail(FLORIA_E_UNSUPPORTED, "more than 2^20 reads in one block");
    const uint64_t tot = roff[n_blocks];
    std::vector<uint32_t> jobs;
    for (uint32_t b = 0; b < n_blocks; ++b) if (cnt[b]) jobs.push_back(b);
    std::stable_sort(jobs.begin(), jobs.end(), [&](uint32_t a, uint32_t b2) { return cnt[a] > cnt[b2]; });
    TR.mark("jobs sorted");
    const bool chunked = SC.chunk_ev != nullptr && SC.n_chunks > 1;
    hipEvent_t group_ev[floria_hip_ctx::MAX_GROUPS] = {};
    const std::vector<uint32_t> group_off = job_groups(ctx, SC, chunked, bc, jobs, group_ev);
    const std::vector<std::vector<uint32_t>> stages = ploidy_stages(ctx, prm, jobs.size(), (uint32_t)group_off.size() - 1);
    uint32_t stage_w = 1;
    for (auto& st : stages) stage_w = std::max<uint32_t>(stage_w, (uint32_t)st.size());

    rc = ensure_binom(ctx, prm->epsilon, len_max); if (rc) return rc;
    if (span_max > fl::HASH_M) return fail(FLORIA_E_UNSUPPORTED, "a block's reads span more than 65536 SNPs");
    rc = ensure_hash(ctx, span_max * nall); if (rc) return rc;

    // ---- device staging of the per-call arrays ----------------------------------------------------------------------
    Carve C;
    const Seg s_rids = C.seg(4ull * tot + 4), s_jobs = C.seg(4ull * jobs.size() + 4), s_bpart = C.seg((uint64_t)(stage_w + 1) * (tot + 16)),        // (+1: the plane of a last-stage beam launch that runs beside the optimise launch below it)
              s_margin = C.seg(8ull * n_blocks * P + 16),
              // zero-initialised, contiguous (ONE memset): partition output, mec / num_alleles / iters, stop-rule state, queue counters, diagnostics
              s_out = C.seg(tot + 16), s_mec = C.seg(8ull * n_blocks * P + 8), s_na = C.seg(8ull * n_blocks * P + 8), s_it = C.seg(4ull * n_blocks * P + 4),
              s_done = C.seg(n_blocks + 4), s_best = C.seg(4ull * n_blocks + 4), s_tried = C.seg(4ull * n_blocks + 4), s_ready = C.seg(4ull * n_blocks + 4),
              s_q = C.seg(8ull * floria_hip_ctx::MAX_LANES * FLORIA_MAX_PLOIDY + 16), s_diag = C.seg(16 + 8 * 64), s_steps = C.seg(16);
    // the partition planes follow: where no launch computes ploidy 1 (ploidy_stages, Knobs::fuse_p1) its plane — every read in partition 0 — is the tail of the same memset
    const bool p1_fused = stages.front().front() == 2;
    const Seg s_planes = C.seg((uint64_t)P * tot + 16);
    const size_t zero_bytes = s_planes.off + (p1_fused ? tot : 0) - s_out.off;
    const Seg s_stop = C.seg(4ull * n_blocks + 4);             // speculative stages: smallest ploidy at which the stop rule is known to break, 0xffffffff = unknown
    rc = C.place(ctx->misc); if (rc) return rc;
    th = T.begin(K_H2D);
    HIPCHK(box_up(C0.at(s_roff), roff.data(), 8ull * (n_blocks + 1), bx_roff));
    if (!jobs.empty()) HIPCHK(box_up(C.at(s_jobs), jobs.data(), 4ull * jobs.size(), bx_jobs));
    HIPCHK(hipMemsetAsync(C.at(s_out), 0, zero_bytes, ctx->stream));
    if (stage_w > 1) HIPCHK(hipMemsetAsync(C.at(s_stop), 0xff, s_stop.bytes, ctx->stream));
    const double inf = std::numeric_limits<double>::infinity();
    T.end(th);
    if (n_blocks) {
        sa.roff = C0.at<const uint64_t>(s_roff); sa.rids = C.at<uint32_t>(s_rids);
        int tk = T.begin(K_SEL);
        hipLaunchKernelGGL(fl::block_reads_kernel<true>, dim3(n_blocks), dim3(64), 0, ctx->stream, sa);
        T.end(tk);
        HIPCHK(hipGetLastError());
        if (!ctx->ev_rids) HIPCHK(hipEventCreateWithFlags(&ctx->ev_rids, hipEventDisableTiming));
        if (!ctx->copy_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        HIPCHK(hipEventRecord(ctx->ev_rids, ctx->stream));
    }

    fl::BlockSet bs{};
    bs.contigs = C0.at<const fl::ContigDev>(s_cdev);
    bs.blk_contig = C0.at<const uint32_t>(s_bc); bs.blk_start = C0.at<const uint32_t>(s_bs); bs.blk_end = C0.at<const uint32_t>(s_be);
    bs.blk_pos0 = C0.at<const uint32_t>(s_p0); bs.blk_span = C0.at<const uint32_t>(s_sp);
    bs.blk_read_off = C0.at<const uint64_t>(s_roff); bs.blk_read = C.at<const uint32_t>(s_rids); bs.n_blocks = n_blocks;

    // ---- reference-arithmetic mode: the iteration order of every read's position set (arith_kernel.h) --------------------------------
    ctx->cur_ord = nullptr; ctx->cur_ord_off = nullptr; ctx->cur_len_max = len_max;
    if (ctx->knobs.arith && n_contigs && SC.orders_in_flight) {
        ctx->cur_ord = ctx->arith_ord.as<uint2>(); ctx->cur_ord_off = ctx->arith_tab.as<uint64_t>() + n_contigs + 1;
    } else if (ctx->knobs.arith && n_contigs) {
        if (SC.n_cells.size() != n_contigs || chunked) return fail(FLORIA_E_INVALID, "internal: the reference-arithmetic mode needs resident contigs");
        int tk = T.begin(K_SEL);
        rc = cell_orders(ctx, bs.contigs, cdev, SC.n_cells, len_max);
        T.end(tk);
        if (rc) return rc;
    }

    // ---- result buffers (allocated first: the read-id lists are copied back while the launch loop runs) -----------------
    floria_block_result* R = (floria_block_result*)calloc(1, sizeof(floria_block_result));
    if (!R) return fail(FLORIA_E_NOMEM, "calloc");
    R->n_blocks = n_blocks; R->max_ploidy = P;
    R->best_ploidy = (uint32_t*)calloc(n_blocks + 1, 4);
    R->ploidies_tried = (uint32_t*)calloc(n_blocks + 1, 4);
    R->read_off = (uint64_t*)calloc(n_blocks + 1, 8);
    const bool lists = !ctx->knobs.s1_no_lists;       // "s1_no_lists": the lists stay where floria_hip_hap_graph and floria_hip_join_paths read them
    R->read_id = lists ? (uint32_t*)g_big.get(4 * (tot + 1)) : nullptr;
    R->part = lists ? (uint8_t*)g_big.get(tot + 1) : nullptr;
    R->mec = (double*)calloc((size_t)n_blocks * P + 1, 8);
    struct ResultGuard { floria_hip_ctx* c; floria_block_result* r; ~ResultGuard() { if (r) { sync_all(c); floria_hip_block_result_free(r); } } } guard{ctx, R};   // every early return below
    if (!R->best_ploidy || !R->ploidies_tried || !R->read_off || (lists && (!R->read_id || !R->part)) || !R->mec) { return fail(FLORIA_E_NOMEM, "malloc"); }
    bool p1_shortcut = false;
    bool all_pk = true;
    for (const fl::ContigDev& cd : cdev) all_pk = all_pk && (cd.n_reads == 0 || cd.cell_pk != nullptr);
    const PhaseShape shape{bs, any_q0, (uint32_t)jobs.size(), tot, n_max, span_max, all_pk};
    const PhaseBufs bufs{C.at<const uint32_t>(s_jobs), C.at<uint8_t>(s_planes), C.at<uint8_t>(s_bpart), C.at<double>(s_mec), C.at<double>(s_na), C.at<uint32_t>(s_it),
                         C.at<uint8_t>(s_done), C.at<uint32_t>(s_best), C.at<uint32_t>(s_tried), C.at<uint32_t>(s_stop), C.at<uint32_t>(s_ready), C.at<uint32_t>(s_q),
                         C.at<double>(s_margin), C.at<uint32_t>(s_diag), C.at<unsigned long long>(s_steps)};
    auto run = nall == 2 ? run_phase<2> : run_phase<4>;
    rc = run(ctx, prm, shape, group_off, stages, chunked ? group_ev : nullptr, bufs, T, p1_shortcut);
    if (rc) { sync_all(ctx); return rc; }
    TR.mark("every launch queued");
    int t_rids = -1;
    if (n_blocks && tot && lists) {     // everything is queued: the copy (pageable destination, the host may block here) overlaps the kernels
        HIPCHK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_rids, 0));
        t_rids = T.begin(K_D2H, ctx->copy_stream);
        hipError_t ce = hipMemcpyAsync(R->read_id, C.at(s_rids), 4ull * tot, hipMemcpyDeviceToHost, ctx->copy_stream);
        T.end(t_rids);
        if (ce != hipSuccess) { sync_all(ctx); return fail(FLORIA_E_DEVICE, hipGetErrorString(ce)); }
    }
    {
        int t = T.begin(K_SEL);
        if (n_blocks) hipLaunchKernelGGL(fl::gather_kernel, dim3(n_blocks), dim3(64), 0, ctx->stream, n_blocks, bs.blk_read_off,
                                         C.at<const uint32_t>(s_best), C.at<const uint8_t>(s_planes), tot, C.at<uint8_t>(s_out));
        T.end(t);
        HIPCHK(hipGetLastError());
    }

    int td = T.begin(K_D2H);
    hipError_t e = hipSuccess;
    uint32_t diag[4] = {0, 0, 0, 0};
    unsigned long long steps = 0;
    double margin = inf;
    if (n_blocks) {
        e = hipMemcpyAsync(R->best_ploidy, C.at(s_best), 4ull * n_blocks, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(R->ploidies_tried, C.at(s_tried), 4ull * n_blocks, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(R->mec, C.at(s_mec), 8ull * n_blocks * P, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && tot && lists) e = hipMemcpyAsync(R->part, C.at(s_out), tot, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(diag, C.at(s_diag), 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&steps, C.at(s_steps), 8, hipMemcpyDeviceToHost, ctx->stream);
    std::vector<double> job_margin((size_t)n_blocks * P + 1, inf);
    if (e == hipSuccess && n_blocks) e = hipMemcpyAsync(job_margin.data(), C.at(s_margin), 8ull * n_blocks * P, hipMemcpyDeviceToHost, ctx->stream);
    T.end(td);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && ctx->copy_stream) e = hipStreamSynchronize(ctx->copy_stream);
    if (e != hipSuccess) { sync_all(ctx); return fail(FLORIA_E_DEVICE, std::string("phase_blocks: ") + hipGetErrorString(e)); }
    TR.mark("results on the host");
    if (diag[1]) { return fail(FLORIA_E_DEVICE, "internal: beam slab free-list underflow"); }
#ifdef FLORIA_PROF
    { unsigned long long prof[64]; (void)hipMemcpy(prof, C.at<char>(s_diag) + 16, sizeof(prof), hipMemcpyDeviceToHost); fprintf(stderr, "[prof]"); for (int i = 0; i < 64; ++i) fprintf(stderr, " %d:%.1fM", i, prof[i] / 1e6); fprintf(stderr, "\n"); }
#endif
    memcpy(R->read_off, roff.data(), 8ull * (n_blocks + 1));
    // the pruning decisions of the (block, ploidy) jobs the reference runs, i.e. ploidy <= ploidies_tried (a speculative stage may have run more)
    for (uint32_t b = 0; b < n_blocks; ++b)
        for (uint32_t p = (p1_shortcut ? 2 : 1); p <= R->ploidies_tried[b]; ++p) margin = std::min(margin, job_margin[(size_t)b * P + p - 1]);
    if (p1_shortcut && !jobs.empty()) margin = std::min(margin, std::fabs(0.0 - std::log(PROB_CUTOFF)));   // the ploidy-1 decisions: p_k - lse == 0
    R->min_prune_margin = margin;
    ctx->timing.beam_ms = T.sum(K_BEAM); ctx->timing.optimize_ms = T.sum(K_OPT); ctx->timing.select_ms = T.sum(K_SEL);
    ctx->timing.beam_union_ms = T.union_ms(K_BEAM); ctx->timing.optimize_union_ms = T.union_ms(K_OPT);
    ctx->timing.h2d_ms = T.sum(K_H2D); ctx->timing.d2h_ms = T.sum(K_D2H); ctx->timing.total_ms = T.span(); ctx->timing.phase_ms = T.sum(K_PHASE);
    ctx->timing.algorithmic_bytes = algo_bytes; ctx->timing.beam_steps = steps;
    ctx->timing.optimize_delta_passes = diag[2]; ctx->timing.optimize_delta_fallbacks = diag[3];
    std::vector<uint32_t> stage_first(P + 2, 0);       // first ploidy of the stage that holds ploidy p
    for (auto& st : stages) for (uint32_t p : st) stage_first[p] = st.front();
    for (uint32_t b = 0; b < n_blocks; ++b) {          // a beam launch for ploidy p phases the blocks still active when p's stage starts (ploidy 1 needs no launch)
        const uint32_t tb = R->ploidies_tried[b];
        uint32_t launches_b = 0;
        for (uint32_t p = 1; p <= P && tb; ++p) if (tb >= stage_first[p] && !(p == 1 && p1_shortcut)) launches_b++;
        ctx->timing.beam_launch_bytes += blk_bytes[b] * launches_b; ctx->timing.jobs += tb;
    }
    ctx->batch_token = R->batch_token = ++ctx->token_counter;
    ctx->last_bs = bs; ctx->last_part = C.at<const uint8_t>(s_out); ctx->last_best = C.at<const uint32_t>(s_best); ctx->last_nall = nall;
    ctx->last_bc = bc; ctx->last_start.assign(blk_start, blk_start + n_blocks); ctx->last_end.assign(blk_end, blk_end + n_blocks);
    guard.r = nullptr;
    *out = R;
    return 0;
}

// "The haplosets of many contigs", as five entry points take them (haploset_stats, haploset_alleles, read_spans, hapq_batch, reassign_batch): group g holds the reads
// grp_read[grp_off[g] .. grp_off[g + 1]) of contig grp_contig[g] (a null grp_contig: all of contig 0).
// check() makes the tests that the host's and the kernels' indexing rests on, each before the first dereference it protects: handles non-null and of this context,
// grp_contig below n_contigs, grp_off ascending, every read id below its contig's n_reads (and a grp_read to read it from).  `who` null: the terse wording of the older
// entry points; else the entry point's name for the wordier one.  The null tests of contigs / grp_off themselves stay with the caller.
// carve() + up() place the tables every kernel of them reads in a Carve the caller goes on with, in this order: the contig table (the caller's own type, as bytes),
// grp_contig, grp_off, grp_read (a segment of `gr_pad` bytes more than the ids), grp_range (null: none).
// ... as the kernels see them: where up() put them, or the arrays of a floria_hip_haplosets handle (nothing is uploaded then)
struct DevGroups { const void* cd = nullptr; const uint32_t* gc = nullptr; const uint64_t* go = nullptr; const uint32_t *gr = nullptr, *rg = nullptr; };
struct GroupTables {
    const void* tab; size_t tab_bytes;
    const uint32_t* grp_contig; const uint64_t* grp_off; const uint32_t *grp_read, *grp_range;
    uint32_t n_groups;
    Seg s_cd{}, s_gc{}, s_go{}, s_gr{}, s_rg{};
    std::vector<uint32_t> zeros;                      // what a null grp_contig stands for

    static int check(const floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig, const uint64_t* grp_off,
                     const uint32_t* grp_read, uint32_t n_groups, const char* who) {
        for (uint32_t i = 0; i < n_contigs; ++i) {
            if (!contigs[i]) return fail(FLORIA_E_INVALID, who ? "null argument" : "bad contig handle");
            if (contigs[i]->ctx != ctx) return fail(FLORIA_E_INVALID, who ? std::string(who) + ": contig " + std::to_string(i) + " belongs to another context" : std::string("bad contig handle"));
        }
        for (uint32_t g = 0; g < n_groups; ++g) {
            const uint32_t c = grp_contig ? grp_contig[g] : 0;
            if (c >= n_contigs) return fail(FLORIA_E_INVALID, "grp_contig out of range");
            if (grp_off[g + 1] < grp_off[g]) return fail(FLORIA_E_INVALID, "grp_off decreases");
            if (grp_off[g + 1] > grp_off[g] && !grp_read) return fail(FLORIA_E_INVALID, "null argument");
            for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) if (grp_read[i] >= contigs[c]->n_reads) return fail(FLORIA_E_INVALID, "group read id out of range");
        }
        return 0;
    }
    void carve(Carve& C, size_t gr_pad) {
        s_cd = C.seg(tab_bytes); s_gc = C.seg(4ull * n_groups); s_go = C.seg(8ull * (n_groups + 1)); s_gr = C.seg(4 * grp_off[n_groups] + gr_pad);
        s_rg = C.seg(grp_range ? 8ull * n_groups : 0);
        if (!grp_contig) zeros.assign(n_groups, 0);
    }
    int up(const Carve& C, hipStream_t st) const {
        HIPCHK(C.up(s_cd, tab, tab_bytes, st)); HIPCHK(C.up(s_gc, grp_contig ? grp_contig : zeros.data(), 4ull * n_groups, st));
        HIPCHK(C.up(s_go, grp_off, 8ull * (n_groups + 1), st)); HIPCHK(C.up(s_gr, grp_read, 4 * grp_off[n_groups], st));
        if (grp_range) HIPCHK(C.up(s_rg, grp_range, 8ull * n_groups, st));
        return 0;
    }
    DevGroups dev(const Carve& C) const { return DevGroups{C.at(s_cd), C.at<const uint32_t>(s_gc), C.at<const uint64_t>(s_go), C.at<const uint32_t>(s_gr), grp_range ? C.at<const uint32_t>(s_rg) : nullptr}; }
};

int stats_core(floria_hip_ctx* ctx, uint32_t A, const uint32_t* grp_range, uint32_t n_groups, GroupTables* G, DevGroups dg, double* out4);
int alleles_core(floria_hip_ctx* ctx, const uint32_t* grp_range, uint32_t n_groups, const uint64_t* pos_off, GroupTables* G, DevGroups dg, uint32_t* counts);
int spans_core(floria_hip_ctx* ctx, uint32_t n_contigs, uint64_t N, uint32_t n_groups, GroupTables* G, DevGroups dg, uint32_t* left, uint32_t* right);
int hapq_core(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const std::vector<uint32_t>& gc, const uint64_t* grp_off, const uint32_t* grp_range,
              uint32_t n_groups, const std::vector<double>& st, const std::vector<uint32_t>& lo, const std::vector<uint32_t>& len, const uint64_t* const* snp_to_genome_pos,
              const uint32_t* n_snps, uint64_t block_length, GroupTables* G, DevGroups dg, uint8_t* hapq, double* rel_err, double* avg_err);

}  // namespace

extern "C" {

int floria_hip_phase_blocks_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                  const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end,
                                  uint32_t n_blocks, const floria_params* prm, floria_block_result** out) {
    if (!ctx || !out || !prm || (n_blocks && (!blk_start || !blk_end || !contigs))) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    S1Contigs SC;
    SC.cdev.resize(n_contigs);
    SC.n_cells.assign(n_contigs, 0);
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t ci = blk_contig ? blk_contig[b] : 0;
        if (ci >= n_contigs || !contigs[ci]) return fail(FLORIA_E_INVALID, "blk_contig out of range");
    }
    for (uint32_t i = 0; i < n_contigs; ++i) if (contigs[i]) {
        if (contigs[i]->ctx != ctx) return fail(FLORIA_E_INVALID, "contig belongs to another context");
        SC.cdev[i] = contigs[i]->dev;
        SC.n_cells[i] = contigs[i]->n_cells;
        SC.len_max = std::max(SC.len_max, contigs[i]->max_len);
        SC.nall = std::max(SC.nall, contigs[i]->n_alleles);
        SC.any_q0 = SC.any_q0 || contigs[i]->has_q0;
    }
    const int rc = s1_core(ctx, SC, blk_contig, blk_start, blk_end, n_blocks, prm, out);
    if (!rc) ctx->last_contigs.assign(contigs, contigs + n_contigs);
    return rc;
}

// S1 straight from host pileups: floria_hip_contig_upload_batch + floria_hip_phase_blocks_batch as ONE pipelined call.  The
// small arrays (read_off, first, last) go first, so find_reads_in_interval and the launch plan are made while the cell arrays
// are still on the wire; the cells travel in chunks of consecutive contigs on the copy stream, each followed by its validate +
// flatten launch, and the blocks of chunk g form job group g, whose kernels start when the chunk has landed.  The PCIe time
// of all but the first chunk hides behind the kernels of the earlier ones.  The launch plan is made for biallelic pileups
// without q = 0 cells (known only once every chunk has been validated); a batch that turns out otherwise is phased again from
// its — by then resident — contigs with the matching kernels, so results never depend on the route.
static int phase_pileups_impl(floria_hip_ctx* ctx, const floria_pileup* pileups, const floria_pileup_packed* pk, uint32_t n_contigs,
                              const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end, uint32_t n_blocks,
                              const floria_params* prm, floria_block_result** out, floria_hip_contig** keep) {
    if (!ctx || !out || !prm || (n_contigs && !pileups && !pk) || (n_blocks && (!blk_start || !blk_end))) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (keep) for (uint32_t i = 0; i < n_contigs; ++i) keep[i] = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    for (uint32_t b = 0; b < n_blocks; ++b) if ((blk_contig ? blk_contig[b] : 0) >= n_contigs) return fail(FLORIA_E_INVALID, "blk_contig out of range");
    if (n_contigs == 0) { S1Contigs SC; return s1_core(ctx, SC, blk_contig, blk_start, blk_end, n_blocks, prm, out); }
    uint64_t cells = 0;
    auto n_reads_of = [&](uint32_t i) { return pk ? pk[i].n_reads : pileups[i].n_reads; };
    for (uint32_t i = 0; i < n_contigs; ++i) { const uint32_t* ro = pk ? pk[i].read_off : pileups[i].read_off; if (n_reads_of(i) && ro) cells += ro[n_reads_of(i)]; }
    // auto: ~0.5 GB of host pileup per chunk, at most 5 (measured on BASELINE config 4, 2.65 GB: 5 chunks, the first one half-size, are best)
    uint32_t want_chunks = ctx->knobs.upload_chunks ? ctx->knobs.upload_chunks : (uint32_t)std::max<uint64_t>(cells * 6 >= (160ull << 20) ? 2 : 1, std::min<uint64_t>(5, cells * 6 / (200ull << 20)));
    // reference-arithmetic mode: a job group's chain of stages is longer (fewer wave slots, the sequential folds), so a group that starts late ends the call late: two chunks
    // (measured on config 4 at -e 0.04, ms per call from packed pinned memory, 1 / 2 / 3 / 5 chunks: 122.2 / 117.7 / 120.5 / 123.4; resident 98; profiles/r06_arith_pipe_timing.txt)
    if (ctx->knobs.arith && !ctx->knobs.upload_chunks) want_chunks = std::min<uint32_t>(want_chunks, 2);
    // (measured, config 4, H2D-inclusive: 500 contigs / 0.66 GB: 2 chunks 60.5 ms, 3-4 chunks 56.5; 1000 contigs / 1.33 GB: 2 chunks 86 ms, 4-5 chunks 77; 2000 contigs: 5 chunks)
    // batches small enough for speculative ploidy stages (s1_core) keep chunk groups x stage width within the hardware queues
    uint32_t chunk_cap = floria_hip_ctx::MAX_GROUPS;
    if (!ctx->knobs.upload_chunks && ctx->knobs.speculate < 0 && prm->max_ploidy >= 3) {
        if (n_blocks <= (uint32_t)ctx->n_cu * 18) chunk_cap = std::max<uint32_t>(1, 10 / prm->max_ploidy);          // (the thresholds of s1_core's stage plan)
        else if (n_blocks <= (uint32_t)ctx->n_cu * 23 && prm->max_ploidy >= 4) chunk_cap = std::max<uint32_t>(1, 10 / std::max<uint32_t>(3, prm->max_ploidy - 3));
    }
    // what an error return releases, each by a guard of its own: the result, the handles once they own the arena (UploadPlan::commit), and — by the plan itself, which
    // stands last so that it waits for the device before any host array a copy reads from goes — the arena until then
    struct Result { floria_block_result* r = nullptr; ~Result() { floria_hip_block_result_free(r); } } res;
    struct Handles { std::vector<floria_hip_contig*> v; ~Handles() { for (auto* h : v) floria_hip_contig_free(h); } } own{std::vector<floria_hip_contig*>(n_contigs, nullptr)};
    std::vector<floria_hip_contig*>& handles = own.v;
    floria_block_result*& R = res.r;
    OrderPlan OP;
    std::vector<fl::ContigDev> pipe_cdev;
    std::vector<uint64_t> pipe_cells;
    UploadPlan UP;
    if (int rc = plan_upload(ctx, pileups, pk, n_contigs, std::min<uint32_t>(std::min(want_chunks, chunk_cap), floria_hip_ctx::MAX_GROUPS), handles.data(), UP)) return rc;
    bool pipelined = UP.all_pinned && UP.n_chunks > 1;
    const bool arith_pipe = pipelined && ctx->knobs.arith != 0;      // reference-arithmetic mode: every chunk's cell orders are computed behind its flatten launch (round 6; until then this mode uploaded the whole batch first)
    const uint64_t order_scratch = 64ull << 20;
    uint64_t pinned_b = 0, staged_b = 0;
    if (pipelined) {
        if (!ctx->copy_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        if (!ctx->flat_stream) {                    // highest priority: when wave slots free up, a waiting flatten launch goes first
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&ctx->flat_stream, hipStreamNonBlocking, hi) != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipStreamCreateWithFlags(&ctx->flat_stream, hipStreamNonBlocking)); }
        }
        for (uint32_t g = 0; g <= UP.n_chunks; ++g) {
            if (!ctx->ev_chunk[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_chunk[g], hipEventDisableTiming));
            if (!ctx->ev_copied[g]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_copied[g], hipEventDisableTiming));
        }
        if (int rc = issue_copies(ctx, UP.small_runs, &pinned_b, &staged_b)) return rc;     // main stream: read_off / first / last + tables
        HIPCHK_AS("pipelined upload: ", issue_tables(ctx, UP, ctx->stream));
        pipe_cdev.resize(n_contigs); pipe_cells.resize(n_contigs);
        for (uint32_t i = 0; i < n_contigs; ++i) { pipe_cdev[i] = UP.dev(i); pipe_cells[i] = UP.cp[i + 1] - UP.cp[i]; }
        size_t ord_cdev_off = 0, ord_todo_words = 0;
        if (arith_pipe) {
            // the order kernels' tables: prefix sums + status word | the contigs' device arrays; the todo lists of the chunks (one count word each) + the emulation's scratch
            order_plan(pipe_cdev, pipe_cells, OP);
            ord_cdev_off = (OP.pre.size() * 8 + 255) & ~(size_t)255;
            ord_todo_words = OP.R_all + UP.n_chunks;
            ctx->ord_epoch = ~0ull;                                                            // (the cached orders are being overwritten)
            if (int rc = ctx->arith_tab.ensure(ord_cdev_off + sizeof(fl::ContigDev) * n_contigs)) return rc;
            if (int rc = ctx->arith_ord.ensure(8 * OP.cells + 16)) return rc;
            if (int rc = ctx->arith_scr.ensure(((8 * ord_todo_words + 255) & ~(size_t)255) + order_scratch)) return rc;
            // (OP / pipe_cdev live until this call returns, behind a sync)
            HIPCHK_AS("pipelined upload: ", hipMemcpyAsync(ctx->arith_tab.p, OP.pre.data(), OP.pre.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK_AS("pipelined upload: ", hipMemcpyAsync(ctx->arith_tab.as<char>() + ord_cdev_off, pipe_cdev.data(), sizeof(fl::ContigDev) * n_contigs, hipMemcpyHostToDevice, ctx->stream));
            for (uint32_t g = 0; g < UP.n_chunks; ++g)                                         // the chunks' todo counters
                HIPCHK_AS("pipelined upload: ", hipMemsetAsync(ctx->arith_scr.as<uint64_t>() + OP.pre[UP.chunk_first[g]] + g, 0, 8, ctx->stream));
        }
        HIPCHK_AS("pipelined upload: ", hipEventRecord(ctx->ev_chunk[UP.n_chunks], ctx->stream));
        HIPCHK_AS("pipelined upload: ", hipStreamWaitEvent(ctx->flat_stream, ctx->ev_chunk[UP.n_chunks], 0));
        for (uint32_t g = 0; g < UP.n_chunks; ++g) {                                           // copy stream: the cells of chunk g, back to back with chunk g+1;
            for (const CopyRun& r : UP.chunk_runs[g]) { pinned_b += r.bytes; HIPCHK_AS("pipelined upload: ", hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyHostToDevice, ctx->copy_stream)); }
            HIPCHK_AS("pipelined upload: ", hipEventRecord(ctx->ev_copied[g], ctx->copy_stream));
            HIPCHK_AS("pipelined upload: ", hipStreamWaitEvent(ctx->flat_stream, ctx->ev_copied[g], 0));       // flatten stream: validate + flatten chunk g
            HIPCHK_AS("pipelined upload: ", launch_flatten(ctx, UP, g, ctx->flat_stream));
            if (arith_pipe) {                                                                  // ... and the iteration orders of its reads' position sets (arith_kernel.h)
                const uint32_t c0 = UP.chunk_first[g], c1 = UP.chunk_first[g + 1];
                if (int rc = order_launch(ctx, OP, (const fl::ContigDev*)(ctx->arith_tab.as<char>() + ord_cdev_off), c0, c1, ctx->arith_scr.as<uint64_t>() + OP.pre[c0] + g,
                                          ctx->arith_scr.as<uint8_t>() + ((8 * ord_todo_words + 255) & ~(size_t)255), order_scratch, 0,
                                          &((const fl::UploadStatus*)(UP.T + UP.t_st) + c0)->max_len, ctx->flat_stream)) return rc;
            }
            HIPCHK_AS("pipelined upload: ", hipEventRecord(ctx->ev_chunk[g], ctx->flat_stream));
        }
        S1Contigs SC;
        SC.cdev = pipe_cdev;
        if (arith_pipe) { SC.n_cells = pipe_cells; SC.orders_in_flight = true; }
        SC.len_max = BINOM_NMAX_CAP; SC.nall = 2; SC.any_q0 = false;                      // optimistic plan, verified below
        SC.contig_chunk = UP.contig_chunk.data(); SC.n_chunks = UP.n_chunks; SC.chunk_ev = ctx->ev_chunk;
        // the compact wire form is on the device in a tenth of the step: what counts then is that the expand / flatten launches of the later chunks are
        // not starved by persistent grids that already own every wave slot.  Measured on config 4 (5 chunks, three runs each, ms per step; chunk -> group):
        // 0|111|2 106.7, 0|11|22 107.7, 00|11|2 108.0, 000|11 108.9, 00|111 108.9, 0|1111 109.3, a group per chunk 109.6, one group 109.4
        if (pk) { SC.chunk_groups = 3; SC.ends_apart = true; }
        if (int rc = s1_core(ctx, SC, blk_contig, blk_start, blk_end, n_blocks, prm, &R)) return rc;
        ctx->last_contigs.assign(handles.begin(), handles.end());
        const floria_timing tm = ctx->timing;
        HIPCHK_AS("upload status: ", hipMemcpy(UP.ust.data(), UP.T + UP.t_st, sizeof(fl::UploadStatus) * n_contigs, hipMemcpyDeviceToHost));
        if (int rc = UP.commit()) return rc;
        if (arith_pipe) {
            uint64_t bad = 0;
            HIPCHK_AS("set-order status: ", hipMemcpy(&bad, ctx->arith_tab.as<uint64_t>() + 2 * (size_t)n_contigs + 2, 8, hipMemcpyDeviceToHost));
            if (int rc = order_bad_read(OP, bad)) return rc;
            ctx->ord_epoch = ctx->upload_epoch; ctx->ord_sig = OP.sig;                      // S2 / the next S1 call over these contigs reuses the orders
        }
        bool plan_ok = true;
        for (auto* h : handles) plan_ok = plan_ok && h->n_alleles == 2 && !h->has_q0;
        for (uint32_t i = 0; i < n_contigs; ++i) plan_ok = plan_ok && !UP.ust[i].no_pk;      // (the plan took every contig's packed cells for granted)
        if (!plan_ok) {                                                                   // rare: phase again with the kernels this batch needs
            floria_hip_block_result_free(R); R = nullptr;
            if (int rc = floria_hip_phase_blocks_batch(ctx, handles.data(), n_contigs, blk_contig, blk_start, blk_end, n_blocks, prm, &R)) return rc;
        } else ctx->timing = tm;
    } else {
        UP.release();                                                                     // (back to the cache: the plain upload takes it from there)
        if (int rc = upload_batch_impl(ctx, pileups, pk, n_contigs, handles.data())) return rc;
        pinned_b = ctx->timing.upload_pinned_bytes; staged_b = ctx->timing.upload_staged_bytes;
        if (int rc = floria_hip_phase_blocks_batch(ctx, handles.data(), n_contigs, blk_contig, blk_start, blk_end, n_blocks, prm, &R)) return rc;
    }
    ctx->timing.upload_pinned_bytes = pinned_b; ctx->timing.upload_staged_bytes = staged_b; ctx->timing.upload_chunks = pipelined ? UP.n_chunks : 1;
    if (keep) { for (uint32_t i = 0; i < n_contigs; ++i) keep[i] = handles[i]; handles.clear(); }
    else { ctx->batch_token = 0; R->batch_token = 0; }     // nothing stays resident (the handles go with this call): no hap graph for this batch
    *out = R; R = nullptr;
    return 0;
}

int floria_hip_phase_pileups_batch(floria_hip_ctx* ctx, const floria_pileup* pileups, uint32_t n_contigs,
                                   const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end, uint32_t n_blocks,
                                   const floria_params* prm, floria_block_result** out, floria_hip_contig** keep) {
    return phase_pileups_impl(ctx, pileups, nullptr, n_contigs, blk_contig, blk_start, blk_end, n_blocks, prm, out, keep);
}
int floria_hip_phase_pileups_batch_packed(floria_hip_ctx* ctx, const floria_pileup_packed* pileups, uint32_t n_contigs,
                                          const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end, uint32_t n_blocks,
                                          const floria_params* prm, floria_block_result** out, floria_hip_contig** keep) {
    return phase_pileups_impl(ctx, nullptr, pileups, n_contigs, blk_contig, blk_start, blk_end, n_blocks, prm, out, keep);
}

int floria_hip_phase_blocks_resident(floria_hip_ctx* ctx, const floria_hip_contig* contig, const uint32_t* blk_start,
                                     const uint32_t* blk_end, uint32_t n_blocks, const floria_params* params,
                                     floria_block_result** out) {
    if (!contig) return fail(FLORIA_E_INVALID, "null contig");
    const floria_hip_contig* arr[1] = {contig};
    return floria_hip_phase_blocks_batch(ctx, arr, 1, nullptr, blk_start, blk_end, n_blocks, params, out);
}

int floria_hip_phase_blocks(floria_hip_ctx* ctx, const floria_pileup* pileup, const uint32_t* blk_start, const uint32_t* blk_end,
                            uint32_t n_blocks, const floria_params* params, floria_block_result** out) {
    floria_hip_contig* c = nullptr;
    int rc = floria_hip_contig_upload(ctx, pileup, &c);
    if (rc) return rc;
    rc = floria_hip_phase_blocks_resident(ctx, c, blk_start, blk_end, n_blocks, params, out);
    floria_hip_contig_free(c);
    return rc;
}

void floria_hip_block_result_free(floria_block_result* r) {
    if (!r) return;
    free(r->best_ploidy); free(r->ploidies_tried); free(r->read_off); g_big.put(r->read_id); g_big.put(r->part); free(r->mec); free(r);
}

// ---- hap-graph nodes + edges on the resident batch ------------------------------------------------
int floria_hip_hap_graph(floria_hip_ctx* ctx, const floria_block_result* res, floria_hap_graph** out) {
    if (!ctx || !res || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (!ctx->batch_token || res->batch_token != ctx->batch_token) return fail(FLORIA_E_INVALID, "the batch is no longer resident: call floria_hip_hap_graph directly after phase_blocks");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t nb = res->n_blocks;
    floria_hap_graph* G = (floria_hap_graph*)calloc(1, sizeof(floria_hap_graph));
    if (!G) return fail(FLORIA_E_NOMEM, "calloc");
    G->n_blocks = nb;
    G->node_off = (uint64_t*)calloc(nb + 1, 8); G->edge_off = (uint64_t*)calloc(nb + 1, 8); G->pred = (int32_t*)calloc(nb + 1, 4);
    uint32_t range_max = 1, pmax = 1;
    {
        std::vector<int32_t> last_of_contig;                    // process_chunks: columns = non-empty blocks in block order (graph_processing.rs:306-323)
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t ci = ctx->last_bc[b];
            if (ci >= last_of_contig.size()) last_of_contig.resize(ci + 1, -1);
            const uint32_t p2 = res->best_ploidy[b];
            G->pred[b] = -1;
            G->node_off[b + 1] = G->node_off[b] + p2;
            G->edge_off[b + 1] = G->edge_off[b];
            if (p2) {
                G->pred[b] = last_of_contig[ci];
                if (G->pred[b] >= 0) G->edge_off[b + 1] += (uint64_t)res->best_ploidy[G->pred[b]] * p2;
                last_of_contig[ci] = (int32_t)b;
                range_max = std::max(range_max, ctx->last_end[b] - ctx->last_start[b] + 1);
                pmax = std::max(pmax, p2);
            }
        }
    }
    const uint64_t n_nodes = G->node_off[nb], n_edges = G->edge_off[nb];
    G->node_cov = (double*)calloc(n_nodes + 1, 8); G->edge_w = (uint32_t*)calloc(n_edges + 1, 4);
    if (!G->node_off || !G->edge_off || !G->pred || !G->node_cov || !G->edge_w) { floria_hip_hap_graph_free(G); return fail(FLORIA_E_NOMEM, "calloc"); }
    if (nb == 0) { *out = G; return 0; }
    const uint32_t A = ctx->last_nall;
    Carve C;
    const Seg s_pred = C.seg(4ull * nb), s_noff = C.seg(8ull * (nb + 1)), s_eoff = C.seg(8ull * (nb + 1)), s_cov = C.seg(8ull * n_nodes + 8), s_ew = C.seg(4ull * n_edges + 4);
    int rc = C.place(ctx->graph_buf);
    const size_t hist_bytes = (size_t)range_max * pmax * A * 8;
    const bool in_lds = hist_bytes <= 40 * 1024;
    uint64_t sort_cap = 1;
    while (sort_cap < (uint64_t)range_max * A) sort_cap <<= 1;
    if (!rc && !in_lds) rc = ctx->graph_hist.ensure((uint64_t)nb * hist_bytes);
    if (!rc && (uint64_t)range_max * A > (uint64_t)fl::GRAPH_SORT_CAP) rc = ctx->graph_sort.ensure((uint64_t)nb * sort_cap * 8);
    if (rc) { floria_hip_hap_graph_free(G); return rc; }
    hipError_t e = C.up(s_pred, G->pred, 4ull * nb, ctx->stream);
    if (e == hipSuccess) e = C.up(s_noff, G->node_off, 8ull * (nb + 1), ctx->stream);
    if (e == hipSuccess) e = C.up(s_eoff, G->edge_off, 8ull * (nb + 1), ctx->stream);
    fl::GraphArgs a{};
    a.bs = ctx->last_bs; a.best_ploidy = ctx->last_best; a.part = ctx->last_part;
    a.pred = C.at<const int32_t>(s_pred); a.node_off = C.at<const uint64_t>(s_noff); a.edge_off = C.at<const uint64_t>(s_eoff);
    a.node_cov = C.at<double>(s_cov); a.edge_w = C.at<uint32_t>(s_ew);
    a.hist_pool = ctx->graph_hist.as<uint64_t>(); a.sort_pool = ctx->graph_sort.as<uint64_t>(); a.sort_cap = sort_cap;
    a.range_max = range_max; a.hist_in_lds = in_lds ? 1 : 0; a.hist_stride = hist_bytes / 8;
    EventTimer T(ctx->stream);
    int tk = T.begin(K_SEL);
    if (e == hipSuccess) {
        if (A == 2) hipLaunchKernelGGL(fl::graph_kernel<2>, dim3(nb), dim3(fl::GRAPH_THREADS), in_lds ? hist_bytes : 0, ctx->stream, a);
        else hipLaunchKernelGGL(fl::graph_kernel<4>, dim3(nb), dim3(fl::GRAPH_THREADS), in_lds ? hist_bytes : 0, ctx->stream, a);
        e = hipGetLastError();
    }
    T.end(tk);
    if (e == hipSuccess && n_nodes) e = hipMemcpyAsync(G->node_cov, C.at(s_cov), 8ull * n_nodes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_edges) e = hipMemcpyAsync(G->edge_w, C.at(s_ew), 4ull * n_edges, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { floria_hip_hap_graph_free(G); return fail(FLORIA_E_DEVICE, std::string("hap_graph: ") + hipGetErrorString(e)); }
    ctx->timing.select_ms = T.sum(K_SEL);
    *out = G;
    return 0;
}
void floria_hip_hap_graph_free(floria_hap_graph* g) {
    if (!g) return;
    free(g->node_off); free(g->node_cov); free(g->pred); free(g->edge_off); free(g->edge_w); free(g);
}

// ---- haploset coverage / error statistics (first half) ---------------------------------------------
int floria_hip_haploset_stats(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                              const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                              const uint32_t* grp_range, uint32_t n_groups, double* out4) {
    if (!ctx || (n_contigs && !contigs) || (n_groups && (!grp_off || !grp_range || !out4))) return fail(FLORIA_E_INVALID, "null argument");
    if (n_groups == 0) return 0;
    if (int rc = GroupTables::check(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, nullptr)) return rc;
    uint32_t A = 2;
    std::vector<fl::ContigDev> cdev(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) { A = std::max(A, contigs[i]->n_alleles); cdev[i] = contigs[i]->dev; }
    GroupTables G{cdev.data(), sizeof(fl::ContigDev) * n_contigs, grp_contig, grp_off, grp_read, grp_range, n_groups};
    return stats_core(ctx, A, grp_range, n_groups, &G, DevGroups{}, out4);
}
}  // extern "C"

namespace {
// The consumers of haplosets behind their validation: the groups come up through `G`, or lie on the device already (`G` null, `dg` = a handle's arrays).
// grp_range and, where given, grp_off are HOST arrays (the caller's, or a handle's header mirror).
int stats_core(floria_hip_ctx* ctx, uint32_t A, const uint32_t* grp_range, uint32_t n_groups, GroupTables* G, DevGroups dg, double* out4) {
    HIPCHK(hipSetDevice(ctx->device));
    ctx->batch_token = 0;                                  // misc is about to be overwritten (floria_hip_hap_graph checks the token)
    std::vector<uint64_t> hoff(n_groups + 1, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t lo = grp_range[2 * g], hi = grp_range[2 * g + 1];
        hoff[g + 1] = hoff[g] + (hi >= lo ? (uint64_t)(hi - lo + 1) * A : 0);
    }
    Carve C;
    if (G) G->carve(C, 4);
    const Seg s_ho = C.seg(8ull * (n_groups + 1)), s_h = C.seg(4ull * hoff[n_groups] + 4), s_out = C.seg(32ull * n_groups);
    if (int rc = C.place(ctx->misc)) return rc;
    if (G) { if (int rc = G->up(C, ctx->stream)) return rc; dg = G->dev(C); }
    HIPCHK(C.up(s_ho, hoff.data(), 8ull * (n_groups + 1), ctx->stream));
    HIPCHK(hipMemsetAsync(C.at(s_h), 0, s_h.bytes, ctx->stream));
    fl::StatsArgs a{};
    a.contigs = (const fl::ContigDev*)dg.cd; a.grp_contig = dg.gc; a.grp_off = dg.go;
    a.grp_read = dg.gr; a.grp_range = dg.rg; a.hist_off = C.at<const uint64_t>(s_ho);
    a.hist = C.at<uint32_t>(s_h); a.out = C.at<double>(s_out); a.n_groups = n_groups;
    if (A == 2) hipLaunchKernelGGL(fl::stats_kernel<2>, dim3(n_groups), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(fl::stats_kernel<4>, dim3(n_groups), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out4, C.at(s_out), 32ull * n_groups, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace
extern "C" {

// ---- self-test of an assumption the kernels make about the hardware: the f32 screen of stable_binom_cdf_p_rev (beam_slab_kernel.h: binom_screen_f32, hardware rcp / log2)
// against the host-libm table, over every (n, k) with n <= n_max.  *max_err_per_n receives max |screen - table| / n; the screen's tolerance assumes <= BINOM_SCREEN_C = 2e-5.
int floria_hip_selftest(floria_hip_ctx* ctx, double epsilon, uint32_t n_max, double* max_err_per_n) {
    if (!ctx || !max_err_per_n || !(epsilon > 0.0 && epsilon < 1.0) || n_max == 0 || n_max > 4096) return fail(FLORIA_E_INVALID, "selftest: context, 0 < epsilon < 1, 1 <= n_max <= 4096");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->batch_token = 0;
    int rc = ensure_binom(ctx, epsilon, n_max); if (rc) return rc;
    rc = ctx->misc.ensure(256); if (rc) return rc;
    double* d_out = ctx->misc.as<double>();
    HIPCHK(hipMemsetAsync(d_out, 0, 8, ctx->stream));
    hipLaunchKernelGGL(fl::binom_screen_selftest_kernel, dim3((n_max + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_binom.as<double>(), n_max,
                       (float)std::log(epsilon), (float)std::log(1.0 - epsilon), (float)epsilon, (float)(1.0 / DIV_FACTOR), d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(max_err_per_n, d_out, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- alignment::realign (alignment.rs:7-64) for the windows the host could not decide --------------------------------------------------------
namespace {
// the exact affine-gap DP: one wavefront per window
hipError_t launch_realign(const floria_hip_ctx* ctx, const fl::RealignArgs& a) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((a.n + 3) / 4, (uint64_t)ctx->n_cu * 32);      // 4 windows per workgroup, grid-stride beyond 8 workgroups per CU
    hipLaunchKernelGGL(fl::realign_kernel, dim3(grid), dim3(256), 0, ctx->stream, a);
    return hipGetLastError();
}
// The one place where a member of the fixed-block walk family becomes a kernel instance: realign_walk_kernel<step = 1 | 2 | 4 | 8, rule = max | sum, tie = right | down>
// (compile-time members: the strip loop of a shift unrolls to step + 8 steps, the rule's reduction and the tie are folded; 59-78 VGPRs, 6-8 waves per SIMD, no scratch in any of the 16).
hipError_t launch_realign_walk(const floria_hip_ctx* ctx, const floria_realign_walk& walk, const fl::RealignArgs& a) {
    const uint32_t per = fl::walk::GROUPS;                                                              // a 16-lane group per window
    const uint32_t grid = (uint32_t)std::min<uint64_t>((a.n + per - 1) / per, (uint64_t)ctx->n_cu * 32);
    return pick<1, 2, 4, 8>(walk.step, [&](auto ST) { return with_bool(walk.rule != 0, [&](auto RU) { return with_bool(walk.tie != 0, [&](auto TI) {
        hipLaunchKernelGGL((fl::realign_walk_kernel<ST, RU ? 1 : 0, TI ? 1 : 0>), dim3(grid), dim3(256), 0, ctx->stream, a);
        return hipGetLastError();
    }); }); });
}
// the members realign_walk_kernel<..> is instantiated for
int walk_member_validate(const floria_realign_walk* walk) {
    if (walk->block != 8 || (walk->step != 1 && walk->step != 2 && walk->step != 4 && walk->step != 8) || walk->rule > 1 || walk->tie > 1)
        return fail(FLORIA_E_INVALID, "floria_realign_walk: block must be 8, step 1, 2, 4 or 8, rule 0 (max) or 1 (sum), tie 0 (right) or 1 (down)");
    return 0;
}
// upload the windows, score them (walk == null: the exact DP), fetch the calls
int realign_windows(floria_hip_ctx* ctx, const uint8_t* read_windows, const uint8_t* ref_windows, const uint8_t* alleles, const uint8_t* n_alleles,
                    uint64_t n, const floria_realign_walk* walk, uint8_t* best, int32_t* score) {
    if (!ctx || (n && (!read_windows || !ref_windows || !alleles || !n_alleles || !best))) return fail(FLORIA_E_INVALID, "null argument");
    if (n == 0) return 0;
    for (uint64_t i = 0; i < n; ++i) if (n_alleles[i] == 0 || n_alleles[i] > FLORIA_MAX_ALLELES) return fail(FLORIA_E_INVALID, "n_alleles must be 1..FLORIA_MAX_ALLELES");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->batch_token = 0;
    Carve C;
    const Seg s_q = C.seg(32 * n), s_r = C.seg(32 * n), s_a = C.seg((size_t)FLORIA_MAX_ALLELES * n), s_n = C.seg(n), s_b = C.seg(n), s_s = C.seg(4 * n);
    int rc = C.place(ctx->misc); if (rc) return rc;
    HIPCHK(C.up(s_q, read_windows, 32 * n, ctx->stream));
    HIPCHK(C.up(s_r, ref_windows, 32 * n, ctx->stream));
    HIPCHK(C.up(s_a, alleles, (size_t)FLORIA_MAX_ALLELES * n, ctx->stream));
    HIPCHK(C.up(s_n, n_alleles, n, ctx->stream));
    fl::RealignArgs a{};
    a.q = C.at<const uint8_t>(s_q); a.r = C.at<const uint8_t>(s_r); a.alleles = C.at<const uint8_t>(s_a); a.n_alleles = C.at<const uint8_t>(s_n);
    a.best = C.at<uint8_t>(s_b); a.score = score ? C.at<int32_t>(s_s) : nullptr; a.n = n;
    HIPCHK(walk ? launch_realign_walk(ctx, *walk, a) : launch_realign(ctx, a));
    HIPCHK(hipMemcpyAsync(best, C.at(s_b), n, hipMemcpyDeviceToHost, ctx->stream));
    if (score) HIPCHK(hipMemcpyAsync(score, C.at(s_s), 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace

int floria_hip_realign(floria_hip_ctx* ctx, const uint8_t* read_windows, const uint8_t* ref_windows, const uint8_t* alleles, const uint8_t* n_alleles,
                       uint64_t n, uint8_t* best, int32_t* score) {
    return realign_windows(ctx, read_windows, ref_windows, alleles, n_alleles, n, nullptr, best, score);
}

int floria_hip_realign_walk(floria_hip_ctx* ctx, const uint8_t* read_windows, const uint8_t* ref_windows, const uint8_t* alleles, const uint8_t* n_alleles,
                            uint64_t n, const floria_realign_walk* walk, uint8_t* best, int32_t* score) {
    if (!walk) return fail(FLORIA_E_INVALID, "null argument");
    if (int rc = walk_member_validate(walk)) return rc;
    return realign_windows(ctx, read_windows, ref_windows, alleles, n_alleles, n, walk, best, score);
}

// ---- frag_from_record (file_reader.rs:661-736) for a batch of alignment records (pileup_kernel.h) -------------------------------------------------
namespace {
// every length the kernels rely on, checked on the host before anything is uploaded or launched
int pileup_validate(const floria_alignments* A, const floria_snp_table* S, bool device_blob = false) {
    const uint32_t n = A->n_records, nc = S->n_contigs;
    if (n && (!A->pos || !A->flags || !A->contig || !A->cigar_off || !A->n_cigar || !A->seq_off || !A->l_seq || !A->qual_off)) return fail(FLORIA_E_INVALID, "floria_alignments: null array");
    if (A->blob_bytes && !A->blob && !device_blob) return fail(FLORIA_E_INVALID, "floria_alignments: null blob");
    if (!S->snp_off) return fail(FLORIA_E_INVALID, "floria_snp_table: null snp_off");
    for (uint32_t c = 0; c < nc; ++c)
        if (S->snp_off[c] > S->snp_off[c + 1]) return fail(FLORIA_E_INVALID, "floria_snp_table: snp_off decreases at contig " + std::to_string(c));
    const uint64_t b = S->snp_off[0], e = S->snp_off[nc];
    if (e > b && (!S->snp_pos || !S->alleles || !S->n_alleles)) return fail(FLORIA_E_INVALID, "floria_snp_table: null array");
    for (uint32_t c = 0; c < nc; ++c)
        for (uint64_t i = S->snp_off[c] + 1; i < S->snp_off[c + 1]; ++i)
            if (S->snp_pos[i] <= S->snp_pos[i - 1])
                return fail(FLORIA_E_INVALID, "floria_snp_table: snp_pos is not strictly ascending at SNP " + std::to_string(i - S->snp_off[c] + 1) + " of contig " + std::to_string(c));
    for (uint64_t i = b; i < e; ++i) {
        if (S->n_alleles[i] == 0) return fail(FLORIA_E_INVALID, "floria_snp_table: n_alleles is 0 at SNP " + std::to_string(i) + " (1.." + std::to_string(FLORIA_MAX_ALLELES) + ")");
        if (S->n_alleles[i] > FLORIA_MAX_ALLELES)
            return fail(FLORIA_E_UNSUPPORTED, "floria_snp_table: " + std::to_string((unsigned)S->n_alleles[i]) + " alleles at SNP " + std::to_string(i) + " (at most " + std::to_string(FLORIA_MAX_ALLELES) + " are supported)");
    }
    const uint64_t B = A->blob_bytes;
    const auto inside = [B](uint64_t off, uint64_t bytes) { return off <= B && bytes <= B - off; };
    for (uint32_t i = 0; i < n; ++i) {
        if (A->contig[i] >= nc) return fail(FLORIA_E_INVALID, "floria_alignments: record " + std::to_string(i) + " names contig " + std::to_string(A->contig[i]) + " of " + std::to_string(nc));
        const uint64_t l = A->l_seq[i];
        const char* what = !inside(A->cigar_off[i], 4ull * A->n_cigar[i]) ? "CIGAR" : !inside(A->seq_off[i], (l + 1) / 2) ? "sequence" : !inside(A->qual_off[i], l) ? "quality" : nullptr;
        if (what) return fail(FLORIA_E_INVALID, std::string("floria_alignments: the ") + what + " bytes of record " + std::to_string(i) + " reach past blob_bytes (" + std::to_string(B) + ")");
    }
    return 0;
}
// the reference sequences of floria_hip_pileup_records_realign: one (possibly empty) sequence per contig of the SNP table
int refs_validate(const floria_ref_seqs* F, const floria_snp_table* S) {
    if (F->n_contigs != S->n_contigs)
        return fail(FLORIA_E_INVALID, "floria_ref_seqs: " + std::to_string(F->n_contigs) + " contigs, the SNP table has " + std::to_string(S->n_contigs));
    if (!F->seq_off) return fail(FLORIA_E_INVALID, "floria_ref_seqs: null seq_off");
    for (uint32_t c = 0; c < F->n_contigs; ++c)
        if (F->seq_off[c] > F->seq_off[c + 1]) return fail(FLORIA_E_INVALID, "floria_ref_seqs: seq_off decreases at contig " + std::to_string(c));
    if (F->seq_off[F->n_contigs] > F->seq_off[0] && !F->seq) return fail(FLORIA_E_INVALID, "floria_ref_seqs: null seq");
    return 0;
}
void* cells_bytes(uint64_t bytes) { return g_big.get((size_t)std::max<uint64_t>(1, bytes)); }      // (library-owned result arrays: floria_hip_record_cells_free)
}  // namespace

void floria_hip_record_cells_free(floria_record_cells* r) {
    if (!r) return;
    g_big.put(r->cell_off); g_big.put(r->snp); g_big.put(r->allele); g_big.put(r->qual); g_big.put(r->seq_pos); g_big.put(r->ref_end); free(r);
}

// Inflated BGZF members on the device (floria_hip_inflate_bgzf): a buffer of its own, so creating, using or freeing it ends no residency.
struct floria_hip_blob {
    floria_hip_ctx* ctx = nullptr;
    DevBuf buf;
    uint64_t bytes = 0;
};

namespace {
// The body of floria_hip_pileup_records and floria_hip_pileup_records_realign: upload, COUNT, offset scan, FILL, download.  With reference sequences (F) the cells'
// alleles are realigned on the device between FILL and the download (realign_gather_kernel.h): DECIDE, one read of its counters, then — when anything is left
// undecided — FILL of the work list, the scoring kernel (walk == null: the exact DP) and the scatter.  Without F nothing of that is allocated, uploaded or launched.
// `resident` (floria_hip_pileup_records_resident): the cell arrays stay where FILL put them; only the per-record arrays come back, with the SNP of every record's
// first / last cell (record_span_kernel) in the places of R->snp / R->seq_pos ([n] instead of [cells]).
// `H` (floria_hip_pileup_records_resident_blob): the record bytes are the handle's, already on the device; the offsets index it and nothing of a blob is uploaded.
int pileup_records_impl(floria_hip_ctx* ctx, const floria_alignments* A_in, const floria_snp_table* S, const floria_ref_seqs* F, const floria_realign_walk* walk,
                        floria_record_cells** out, floria_realign_counts* counts, bool resident = false, const floria_hip_blob* H = nullptr) {
    if (!ctx || !A_in || !S || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    ctx->res_token = 0; ctx->res_summary = nullptr;      // pile_in / pile_out are about to be rewritten: a residency ends here
    if (counts) *counts = floria_realign_counts{};
    floria_alignments A_view = *A_in;
    if (H) {
        if (H->ctx != ctx) return fail(FLORIA_E_INVALID, "the blob belongs to another context");
        if (A_in->blob) return fail(FLORIA_E_INVALID, "floria_alignments: blob must be NULL beside a blob handle (the offsets index the handle)");
        A_view.blob_bytes = H->bytes;
    }
    const floria_alignments* A = &A_view;
    if (int rc = pileup_validate(A, S, H != nullptr)) return rc;
    if (F) { if (int rc = refs_validate(F, S)) return rc; }
    if (walk) { if (int rc = walk_member_validate(walk)) return rc; }
    const uint32_t n = A->n_records, nc = S->n_contigs;
    floria_record_cells* R = (floria_record_cells*)calloc(1, sizeof(floria_record_cells));
    if (!R) return fail(FLORIA_E_NOMEM, "calloc");
    uint64_t hc[fl::RG_N_COUNTS] = {};      // the realignment's counters come back here: declared before `guard`, which synchronises the stream on every early return, so no copy outlives it
    // (an error return: nothing may still be copying into the arrays when they are released)
    struct Guard { floria_record_cells* r; hipStream_t st; ~Guard() { if (r) { (void)hipStreamSynchronize(st); floria_hip_record_cells_free(r); } } } guard{R, ctx->stream};
    R->n_records = n;
    R->cell_off = (uint64_t*)cells_bytes(8ull * ((uint64_t)n + 1)); R->ref_end = (int64_t*)cells_bytes(8ull * n);
    if (!R->cell_off || !R->ref_end) return fail(FLORIA_E_NOMEM, "malloc");
    R->cell_off[0] = 0;
    uint64_t total = 0;
    const auto alloc_cells = [R, resident, n](uint64_t t) {
        if (resident) { R->snp = (uint32_t*)cells_bytes(4ull * n); R->seq_pos = (uint32_t*)cells_bytes(4ull * n); return R->snp && R->seq_pos ? 0 : fail(FLORIA_E_NOMEM, "malloc"); }
        R->snp = (uint32_t*)cells_bytes(4 * t); R->allele = (uint8_t*)cells_bytes(t); R->qual = (uint8_t*)cells_bytes(t); R->seq_pos = (uint32_t*)cells_bytes(4 * t);
        return R->snp && R->allele && R->qual && R->seq_pos ? 0 : fail(FLORIA_E_NOMEM, "malloc");
    };
    ctx->timing = floria_timing{};
    if (n == 0) { if (int rc = alloc_cells(0)) return rc; }
    else {
        HIPCHK(hipSetDevice(ctx->device));
        const uint64_t snp_b = S->snp_off[0], n_snps = S->snp_off[nc] - snp_b;
        const uint32_t n_tiles = (n + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
        Carve C;
        const Seg s_blob = C.seg(H ? 0 : A->blob_bytes), s_pos = C.seg(4ull * n), s_flag = C.seg(2ull * n), s_ctg = C.seg(4ull * n), s_co = C.seg(8ull * n), s_nc = C.seg(4ull * n),
                  s_so = C.seg(8ull * n), s_ls = C.seg(4ull * n), s_qo = C.seg(8ull * n), s_soff = C.seg(8ull * (nc + 1)), s_sp = C.seg(8 * n_snps), s_al = C.seg(4 * n_snps),
                  s_na = C.seg(n_snps), s_off = C.seg(8ull * ((uint64_t)n + 1)), s_tile = C.seg(8ull * n_tiles), s_re = C.seg(8ull * n);
        const Seg s_f1 = C.seg(resident ? 4ull * n : 0), s_l1 = C.seg(resident ? 4ull * n : 0);
        const uint64_t ref_b = F ? F->seq_off[0] : 0, ref_bytes = F ? F->seq_off[nc] - ref_b : 0;
        const Seg s_roff = C.seg(F ? 8ull * (nc + 1) : 0), s_ref = C.seg(ref_bytes), s_cnt = C.seg(F ? 8ull * fl::RG_N_COUNTS : 0);
        if (int rc = C.place(ctx->pile_in)) return rc;
        EventTimer T(ctx->stream);
        uint64_t pinned_b = 0, staged_b = 0;
        {
            std::vector<CopyRun> runs;
            const auto up = [&](Seg s, const void* src) { if (s.bytes) runs.push_back({(const char*)src, C.at<char>(s), s.bytes}); };
            up(s_blob, A->blob); up(s_pos, A->pos); up(s_flag, A->flags); up(s_ctg, A->contig); up(s_co, A->cigar_off); up(s_nc, A->n_cigar); up(s_so, A->seq_off);
            up(s_ls, A->l_seq); up(s_qo, A->qual_off); up(s_soff, S->snp_off);
            if (n_snps) { up(s_sp, S->snp_pos + snp_b); up(s_al, S->alleles + 4 * snp_b); up(s_na, S->n_alleles + snp_b); }
            if (F) { up(s_roff, F->seq_off); if (ref_bytes) up(s_ref, F->seq + ref_b); }
            const int t = T.begin(K_H2D);
            if (int rc = issue_copies(ctx, runs, &pinned_b, &staged_b)) return rc;
            T.end(t);
        }
        fl::PileupArgs a{};
        a.blob = H ? H->buf.as<const uint8_t>() : C.at<const uint8_t>(s_blob); a.pos = C.at<const int32_t>(s_pos); a.flags = C.at<const uint16_t>(s_flag); a.contig = C.at<const uint32_t>(s_ctg);
        a.cigar_off = C.at<const uint64_t>(s_co); a.n_cigar = C.at<const uint32_t>(s_nc); a.seq_off = C.at<const uint64_t>(s_so); a.l_seq = C.at<const uint32_t>(s_ls);
        a.qual_off = C.at<const uint64_t>(s_qo); a.snp_off = C.at<const uint64_t>(s_soff);
        // (the table travels from its first used entry: the kernels index it with the caller's offsets)
        a.snp_pos = C.at<const int64_t>(s_sp) - snp_b; a.alleles = C.at<const uint8_t>(s_al) - 4 * snp_b; a.n_alleles = C.at<const uint8_t>(s_na) - snp_b;
        a.cell_off = C.at<uint64_t>(s_off); a.ref_end = C.at<int64_t>(s_re); a.n_records = n;
        const uint32_t grid = items_grid(ctx, n, 4);      // one wavefront per record
        int t = T.begin(K_PILEUP);
        hipLaunchKernelGGL(fl::pileup_walk_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        launch_offset_scan(ctx, a.cell_off, C.at<uint64_t>(s_tile), n);
        HIPCHK(hipGetLastError());
        T.end(t);
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(R->cell_off, a.cell_off, 8ull * ((uint64_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        total = R->cell_off[n];
        if (int rc = alloc_cells(total)) return rc;
        Carve O;
        const Seg o_snp = O.seg(4 * total), o_al = O.seg(total), o_q = O.seg(total), o_sp = O.seg(4 * total), o_und = O.seg(F ? total : 0);
        if (int rc = O.place(ctx->pile_out)) return rc;
        a.snp = O.at<uint32_t>(o_snp); a.allele = O.at<uint8_t>(o_al); a.qual = O.at<uint8_t>(o_q); a.seq_pos = O.at<uint32_t>(o_sp);
        t = T.begin(K_PILEUP);
        hipLaunchKernelGGL(fl::pileup_walk_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        T.end(t);
        if (F && total) {
            fl::RealignGatherArgs r{};
            r.blob = a.blob; r.contig = a.contig; r.seq_off = a.seq_off; r.l_seq = a.l_seq; r.cell_off = a.cell_off; r.snp_off = a.snp_off; r.snp_pos = a.snp_pos;
            r.alleles = a.alleles; r.n_alleles = a.n_alleles; r.ref_off = C.at<const uint64_t>(s_roff); r.ref_seq = C.at<const uint8_t>(s_ref) - ref_b;
            r.snp = a.snp; r.seq_pos = a.seq_pos; r.allele = a.allele; r.undecided = O.at<uint8_t>(o_und); r.counts = C.at<uint64_t>(s_cnt);
            r.n_cells = total; r.n_records = n;
            const uint32_t ggrid = items_grid(ctx, total, 8);      // 8 cells per workgroup and trip
            t = T.begin(K_PILEUP);
            HIPCHK(hipMemsetAsync(r.counts, 0, 8ull * fl::RG_N_COUNTS, ctx->stream));
            hipLaunchKernelGGL(fl::realign_decide_kernel, dim3(ggrid), dim3(256), 0, ctx->stream, r);
            HIPCHK(hipGetLastError());
            T.end(t);
            t = T.begin(K_D2H);
            HIPCHK(hipMemcpyAsync(hc, r.counts, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));      // the work list is sized from the count, not from 69 B x cells
            T.end(t);
            HIPCHK(hipStreamSynchronize(ctx->stream));
            const uint64_t n_work = hc[fl::RG_SCORED];
            if (n_work > total) return fail(FLORIA_E_DEVICE, "realign: more undecided cells than cells");
            if (n_work) {
                Carve W;
                const Seg w_q = W.seg(32 * n_work), w_r = W.seg(32 * n_work), w_a = W.seg((size_t)FLORIA_MAX_ALLELES * n_work), w_n = W.seg(n_work), w_b = W.seg(n_work),
                          w_c = W.seg(8 * n_work);
                ctx->batch_token = 0;                                   // misc is about to be overwritten: a resident S1 batch is gone (floria_hip_hap_graph checks the token)
                if (int rc = W.place(ctx->misc)) return rc;
                r.wq = W.at<uint8_t>(w_q); r.wr = W.at<uint8_t>(w_r); r.wal = W.at<uint8_t>(w_a); r.wna = W.at<uint8_t>(w_n); r.wcell = W.at<uint64_t>(w_c); r.cap = n_work;
                fl::RealignArgs ra{};
                ra.q = r.wq; ra.r = r.wr; ra.alleles = r.wal; ra.n_alleles = r.wna; ra.best = W.at<uint8_t>(w_b); ra.score = nullptr; ra.n = n_work;
                t = T.begin(K_PILEUP);
                hipLaunchKernelGGL(fl::realign_fill_kernel, dim3(ggrid), dim3(256), 0, ctx->stream, r);
                HIPCHK(hipGetLastError());
                HIPCHK(walk ? launch_realign_walk(ctx, *walk, ra) : launch_realign(ctx, ra));
                const uint32_t sgrid = items_grid(ctx, n_work, 256);
                hipLaunchKernelGGL(fl::realign_scatter_kernel, dim3(sgrid), dim3(256), 0, ctx->stream, (const uint8_t*)ra.best, (const uint64_t*)r.wcell, n_work, r.allele, r.counts);
                HIPCHK(hipGetLastError());
                T.end(t);
            }
        }
        if (resident) {
            t = T.begin(K_PILEUP);
            hipLaunchKernelGGL(fl::record_span_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint64_t*)a.cell_off, (const uint32_t*)a.snp, C.at<uint32_t>(s_f1), C.at<uint32_t>(s_l1), n);
            HIPCHK(hipGetLastError());
            T.end(t);
        }
        t = T.begin(K_D2H);
        if (F && total && hc[fl::RG_SCORED]) HIPCHK(hipMemcpyAsync(hc, C.at<uint64_t>(s_cnt), sizeof hc, hipMemcpyDeviceToHost, ctx->stream));      // (the scatter's share of `changed`)
        if (resident) {
            HIPCHK(hipMemcpyAsync(R->snp, C.at(s_f1), 4ull * n, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(R->seq_pos, C.at(s_l1), 4ull * n, hipMemcpyDeviceToHost, ctx->stream));
        } else if (total) {
            HIPCHK(hipMemcpyAsync(R->snp, a.snp, 4 * total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(R->allele, a.allele, total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(R->qual, a.qual, total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(R->seq_pos, a.seq_pos, 4 * total, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipMemcpyAsync(R->ref_end, a.ref_end, 8ull * n, hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        T.publish(ctx->timing);
        ctx->timing.upload_pinned_bytes = pinned_b; ctx->timing.upload_staged_bytes = staged_b;
        if (F && total) {
            if (hc[fl::RG_APPENDED] != hc[fl::RG_SCORED]) return fail(FLORIA_E_DEVICE, "realign: the work list holds another number of windows than were counted");
            if (counts) { counts->in_bounds = hc[fl::RG_IN_BOUNDS]; counts->shortcut = hc[fl::RG_SHORTCUT]; counts->scored = hc[fl::RG_SCORED]; counts->changed = hc[fl::RG_CHANGED]; }
        }
        if (counts) counts->cells = total;
        if (resident) {
            ctx->res_contig.assign(A->contig, A->contig + n); ctx->res_n_contigs = nc;
            ctx->res_cell_off = a.cell_off; ctx->res_snp = a.snp; ctx->res_allele = a.allele; ctx->res_qual = a.qual; ctx->res_seq_pos = a.seq_pos;
        }
    }
    if (resident && n == 0) { ctx->res_contig.clear(); ctx->res_n_contigs = nc; ctx->res_cell_off = nullptr; ctx->res_snp = nullptr; ctx->res_allele = nullptr; ctx->res_qual = nullptr; ctx->res_seq_pos = nullptr; }
    guard.r = nullptr;
    *out = R;
    return 0;
}
}  // namespace

int floria_hip_pileup_records(floria_hip_ctx* ctx, const floria_alignments* A, const floria_snp_table* S, floria_record_cells** out) {
    return pileup_records_impl(ctx, A, S, nullptr, nullptr, out, nullptr);
}

int floria_hip_pileup_records_realign(floria_hip_ctx* ctx, const floria_alignments* A, const floria_snp_table* S, const floria_ref_seqs* F, const floria_realign_walk* walk,
                                      floria_record_cells** out, floria_realign_counts* counts) {
    if (!F) return fail(FLORIA_E_INVALID, "null argument");
    return pileup_records_impl(ctx, A, S, F, walk, out, counts);
}

// ---- records -> cells -> resident contigs (assemble_kernel.h) ------------------------------------------------------------------------------------------------
int floria_hip_pileup_records_resident(floria_hip_ctx* ctx, const floria_alignments* A, const floria_snp_table* S, const floria_ref_seqs* F, const floria_realign_walk* walk,
                                       floria_record_summary** out) {
    if (!out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    floria_record_summary* Y = (floria_record_summary*)calloc(1, sizeof(floria_record_summary));
    if (!Y) return fail(FLORIA_E_NOMEM, "calloc");
    floria_record_cells* R = nullptr;
    if (int rc = pileup_records_impl(ctx, A, S, F, walk, &R, &Y->counts, true)) { free(Y); return rc; }
    // (the impl leaves the records' first / last SNPs in the [n] arrays it allocated for R->snp / R->seq_pos; allele and qual were never allocated)
    Y->n_records = R->n_records; Y->cell_off = R->cell_off; Y->first_snp = R->snp; Y->last_snp = R->seq_pos; Y->ref_end = R->ref_end;
    free(R);
    Y->token = ++ctx->token_counter;
    ctx->res_token = Y->token; ctx->res_summary = Y;
    *out = Y;
    return 0;
}

void floria_hip_record_summary_free(floria_record_summary* s) {
    if (!s) return;
    g_big.put(s->cell_off); g_big.put(s->first_snp); g_big.put(s->last_snp); g_big.put(s->ref_end); free(s);
}

// ---- BGZF members inflated on the device, and the record table of the inflated bytes (inflate_kernel.h) --------------------------------------------------------------
namespace {
const char* inflate_reason(uint32_t st) {
    static const char* const R[fl::INF_N_STATUS] = {"ok", "bits ran out", "reserved block type", "LEN/NLEN mismatch", "over-subscribed code lengths", "incomplete code lengths",
                                                    "distance beyond the bytes produced", "output longer than ISIZE", "output shorter than ISIZE", "CRC mismatch", "invalid code",
                                                    "step bound reached"};
    return st < fl::INF_N_STATUS ? R[st] : "unknown status";
}
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
}  // namespace

int floria_hip_inflate_bgzf(floria_hip_ctx* ctx, const uint8_t* file, uint64_t n_bytes, const uint64_t* member_off, const uint32_t* member_bytes, uint32_t n, floria_hip_blob** out) {
    if (!ctx || !out || (n && (!file || !member_off || !member_bytes))) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    // the host part: every member's gzip header and trailer, before anything is uploaded or launched
    std::vector<uint64_t> pay_off(n), out_off((size_t)n + 1, 0);
    std::vector<uint32_t> pay_bytes(n), crc(n);
    uint64_t lo = n_bytes, hi = 0;
    for (uint32_t m = 0; m < n; ++m) {
        const std::string who = "BGZF member " + std::to_string(m);
        const uint64_t off = member_off[m], mb = member_bytes[m];
        if (off > n_bytes || mb > n_bytes - off) return fail(FLORIA_E_INVALID, who + ": bytes " + std::to_string(off) + " + " + std::to_string(mb) + " reach past n_bytes (" + std::to_string(n_bytes) + ")");
        if (mb < 12 + 6 + 8) return fail(FLORIA_E_INVALID, who + ": " + std::to_string(mb) + " bytes are less than a BGZF header and trailer");
        const uint8_t* p = file + off;
        if (p[0] != 31 || p[1] != 139) return fail(FLORIA_E_INVALID, who + ": no gzip magic");
        if (p[2] != 8) return fail(FLORIA_E_INVALID, who + ": compression method " + std::to_string((unsigned)p[2]) + " (8 = DEFLATE)");
        if (p[3] != 4) return fail(FLORIA_E_INVALID, who + ": gzip flags " + std::to_string((unsigned)p[3]) + " (BGZF sets FEXTRA alone)");
        const uint64_t xlen = le16(p + 10);
        if (12 + xlen + 8 > mb) return fail(FLORIA_E_INVALID, who + ": the extra field (" + std::to_string(xlen) + " bytes) reaches past the member");
        uint64_t x = 12, bsize = 0;
        while (x + 4 <= 12 + xlen) {
            const uint32_t slen = le16(p + x + 2);
            if (p[x] == 66 && p[x + 1] == 67 && slen == 2 && x + 6 <= 12 + xlen) { bsize = (uint64_t)le16(p + x + 4) + 1; break; }
            x += 4 + (uint64_t)slen;
        }
        if (!bsize) return fail(FLORIA_E_INVALID, who + ": no BC subfield in the extra field");
        if (bsize != mb) return fail(FLORIA_E_INVALID, who + ": BSIZE says " + std::to_string(bsize) + " bytes, member_bytes " + std::to_string(mb));
        const uint32_t isize = le32(p + mb - 4);
        if (isize > fl::INF_MAX_OUT) return fail(FLORIA_E_UNSUPPORTED, who + ": ISIZE " + std::to_string(isize) + " is more than 65536: a gzip file that is not BGZF");
        pay_off[m] = off + 12 + xlen; pay_bytes[m] = (uint32_t)(mb - 12 - xlen - 8);
        crc[m] = le32(p + mb - 8);
        out_off[m + 1] = out_off[m] + isize;
        lo = std::min(lo, off); hi = std::max(hi, off + mb);
    }
    floria_hip_blob* B = new (std::nothrow) floria_hip_blob();
    if (!B) return fail(FLORIA_E_NOMEM, "new");
    struct Guard { floria_hip_blob* b; hipStream_t st; ~Guard() { if (b) { (void)hipStreamSynchronize(st); b->buf.release(); delete b; } } } guard{B, ctx->stream};
    B->ctx = ctx; B->bytes = out_off[n];
    ctx->timing = floria_timing{};
    HIPCHK(hipSetDevice(ctx->device));
    if (int rc = B->buf.ensure(B->bytes + 256)) return rc;
    if (n) {
        lo &= ~(uint64_t)3;                                  // the kernel reads the file as aligned words
        const uint64_t span = hi - lo, span_words = (span + 3) / 4;
        for (uint32_t m = 0; m < n; ++m) pay_off[m] -= lo;
        Carve C;
        const Seg s_file = C.seg(4 * span_words), s_po = C.seg(8ull * n), s_pb = C.seg(4ull * n), s_oo = C.seg(8ull * ((uint64_t)n + 1)), s_crc = C.seg(4ull * n), s_st = C.seg(4ull * n);
        if (int rc = C.place(ctx->inf_in)) return rc;
        EventTimer T(ctx->stream);
        uint64_t pinned_b = 0, staged_b = 0;
        {
            std::vector<CopyRun> runs;
            runs.push_back({(const char*)file + lo, C.at<char>(s_file), (size_t)span});
            runs.push_back({(const char*)pay_off.data(), C.at<char>(s_po), 8 * (size_t)n}); runs.push_back({(const char*)pay_bytes.data(), C.at<char>(s_pb), 4 * (size_t)n});
            runs.push_back({(const char*)out_off.data(), C.at<char>(s_oo), 8 * ((size_t)n + 1)}); runs.push_back({(const char*)crc.data(), C.at<char>(s_crc), 4 * (size_t)n});
            const int t = T.begin(K_H2D);
            if (int rc = issue_copies(ctx, runs, &pinned_b, &staged_b)) return rc;
            T.end(t);
        }
        fl::InflateArgs a{};
        a.file = C.at<const uint8_t>(s_file); a.file_words = span_words; a.pay_off = C.at<const uint64_t>(s_po); a.pay_bytes = C.at<const uint32_t>(s_pb);
        a.out_off = C.at<const uint64_t>(s_oo); a.blob = B->buf.as<uint8_t>(); a.status = C.at<uint32_t>(s_st); a.n_members = n;
        const uint32_t slots = ctx->inflate_slots ? ctx->inflate_slots : 2 * (uint32_t)ctx->n_cu;
        HIPCHK(hipFuncSetAttribute((const void*)fl::inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl::INF_LDS_BYTES));
        int t = T.begin(K_PILEUP);
        hipLaunchKernelGGL(fl::inflate_kernel, dim3(std::min(n, slots)), dim3(64), fl::INF_LDS_BYTES, ctx->stream, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(fl::inflate_crc_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint8_t*)a.blob, a.out_off, C.at<const uint32_t>(s_crc), a.status, n);
        HIPCHK(hipGetLastError());
        T.end(t);
        std::vector<uint32_t> status(n);
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(status.data(), a.status, 4ull * n, hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        T.publish(ctx->timing);
        ctx->timing.upload_pinned_bytes = pinned_b; ctx->timing.upload_staged_bytes = staged_b;
        for (uint32_t m = 0; m < n; ++m)
            if (status[m] != fl::INF_OK) return fail(FLORIA_E_INVALID, "BGZF member " + std::to_string(m) + ": " + inflate_reason(status[m]));
    }
    guard.b = nullptr;
    *out = B;
    return 0;
}

uint64_t floria_hip_blob_bytes(const floria_hip_blob* b) { return b ? b->bytes : 0; }

int floria_hip_blob_download(const floria_hip_blob* b, uint64_t off, void* dst, uint64_t bytes) {
    if (!b || (bytes && !dst)) return fail(FLORIA_E_INVALID, "null argument");
    if (off > b->bytes || bytes > b->bytes - off) return fail(FLORIA_E_INVALID, "blob download: bytes " + std::to_string(off) + " + " + std::to_string(bytes) + " reach past the blob (" + std::to_string(b->bytes) + ")");
    if (!bytes) return 0;
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpy(dst, b->buf.as<char>() + off, bytes, hipMemcpyDeviceToHost));
    return 0;
}

void floria_hip_blob_free(floria_hip_blob* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    b->buf.release();
    delete b;
}

void floria_hip_blob_records_free(floria_blob_records* r) {
    if (!r) return;
    for (void* p : {(void*)r->chain_rec_off, (void*)r->chain_stop, (void*)r->chain_why, (void*)r->offset, (void*)r->block_size, (void*)r->ref_id, (void*)r->pos, (void*)r->l_seq, (void*)r->cigar0,
                    (void*)r->flag, (void*)r->n_cigar_op, (void*)r->mapq, (void*)r->l_read_name, (void*)r->name_off, (void*)r->names}) g_big.put(p);
    free(r);
}

static_assert(FLORIA_CHAIN_CUT_TAIL == fl::CHAIN_CUT_TAIL && FLORIA_CHAIN_ONE_REF == fl::CHAIN_ONE_REF, "chain flags out of sync");

int floria_hip_blob_records(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* begin, const uint64_t* end, uint32_t nch, floria_blob_records** out) {
    return floria_hip_blob_records_opt(ctx, blob, begin, end, nch, 0, out);
}

int floria_hip_blob_records_opt(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* begin, const uint64_t* end, uint32_t nch, uint32_t flags, floria_blob_records** out) {
    if (!ctx || !blob || !out || (nch && (!begin || !end))) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (blob->ctx != ctx) return fail(FLORIA_E_INVALID, "the blob belongs to another context");
    if (flags & ~(uint32_t)(FLORIA_CHAIN_CUT_TAIL | FLORIA_CHAIN_ONE_REF)) return fail(FLORIA_E_INVALID, "blob_records: flags " + std::to_string(flags) + " (FLORIA_CHAIN_CUT_TAIL | FLORIA_CHAIN_ONE_REF)");
    for (uint32_t c = 0; c < nch; ++c)
        if (begin[c] > end[c] || end[c] > blob->bytes)
            return fail(FLORIA_E_INVALID, "blob_records: chain " + std::to_string(c) + " [" + std::to_string(begin[c]) + ", " + std::to_string(end[c]) + ") is no range of the blob (" + std::to_string(blob->bytes) + " bytes)");
    floria_blob_records* R = (floria_blob_records*)calloc(1, sizeof(floria_blob_records));
    if (!R) return fail(FLORIA_E_NOMEM, "calloc");
    struct Guard { floria_blob_records* r; hipStream_t st; ~Guard() { if (r) { (void)hipStreamSynchronize(st); floria_hip_blob_records_free(r); } } } guard{R, ctx->stream};
    R->n_chains = nch;
    R->chain_rec_off = (uint64_t*)cells_bytes(8ull * ((uint64_t)nch + 1)); R->chain_stop = (uint64_t*)cells_bytes(8ull * nch); R->chain_why = (uint32_t*)cells_bytes(4ull * nch);
    if (!R->chain_rec_off || !R->chain_stop || !R->chain_why) return fail(FLORIA_E_NOMEM, "malloc");
    R->chain_rec_off[0] = 0;
    ctx->timing = floria_timing{};
    uint64_t N = 0, name_bytes = 0;
    EventTimer T(ctx->stream);
    fl::RecordArgs q{};
    if (nch) {
        HIPCHK(hipSetDevice(ctx->device));
        const uint32_t n_tiles = (nch + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
        Carve C;
        const Seg s_b = C.seg(8ull * nch), s_e = C.seg(8ull * nch), s_cnt = C.seg(8ull * ((uint64_t)nch + 1)), s_stop = C.seg(8ull * nch), s_st = C.seg(4ull * nch), s_why = C.seg(4ull * nch), s_tile = C.seg(8ull * n_tiles);
        if (int rc = C.place(ctx->rec_in)) return rc;
        int t = T.begin(K_H2D);
        HIPCHK(C.up(s_b, begin, 8ull * nch, ctx->stream)); HIPCHK(C.up(s_e, end, 8ull * nch, ctx->stream));
        T.end(t);
        fl::ChainArgs a{};
        a.blob = blob->buf.as<const uint8_t>(); a.blob_bytes = blob->bytes; a.begin = C.at<const uint64_t>(s_b); a.end = C.at<const uint64_t>(s_e);
        a.count = C.at<uint64_t>(s_cnt); a.stop = C.at<uint64_t>(s_stop); a.status = C.at<uint32_t>(s_st); a.why = C.at<uint32_t>(s_why); a.n_chains = nch; a.flags = flags;
        t = T.begin(K_PILEUP);
        hipLaunchKernelGGL(fl::blob_chain_kernel<false>, dim3((nch + 255) / 256), dim3(256), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        launch_offset_scan(ctx, a.count, C.at<uint64_t>(s_tile), nch);
        HIPCHK(hipGetLastError());
        T.end(t);
        std::vector<uint32_t> status(nch);
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(R->chain_rec_off, a.count, 8ull * ((uint64_t)nch + 1), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(R->chain_stop, a.stop, 8ull * nch, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(status.data(), a.status, 4ull * nch, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(R->chain_why, a.why, 4ull * nch, hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (uint32_t c = 0; c < nch; ++c)
            if (status[c] != fl::CHAIN_OK)
                return fail(FLORIA_E_INVALID, "blob_records: chain " + std::to_string(c) + " stopped at offset " + std::to_string(R->chain_stop[c]) + ": " +
                                                  (status[c] == fl::CHAIN_SHORT ? "a block_size below the 32 fixed bytes of a record" : "a record that runs past the chain's end (" + std::to_string(end[c]) + ")"));
        N = R->chain_rec_off[nch];
        if (N >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "blob_records: 2^32 and more records");
        if (N) {
            const uint32_t r_tiles = ((uint32_t)N + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
            Carve O;
            const Seg o_off = O.seg(8 * N), o_bs = O.seg(4 * N), o_ref = O.seg(4 * N), o_pos = O.seg(4 * N), o_ls = O.seg(4 * N), o_cg = O.seg(4 * N), o_fl = O.seg(2 * N), o_nc = O.seg(2 * N),
                      o_mq = O.seg(N), o_ln = O.seg(N), o_no = O.seg(8 * (N + 1)), o_tile = O.seg(8ull * r_tiles);
            if (int rc = O.place(ctx->rec_out)) return rc;
            a.rec_off = O.at<uint64_t>(o_off);
            q.blob = a.blob; q.blob_bytes = a.blob_bytes; q.rec_off = a.rec_off; q.ref_id = O.at<int32_t>(o_ref); q.pos = O.at<int32_t>(o_pos); q.block_size = O.at<uint32_t>(o_bs);
            q.l_seq = O.at<uint32_t>(o_ls); q.cigar0 = O.at<uint32_t>(o_cg); q.flag = O.at<uint16_t>(o_fl); q.n_cigar_op = O.at<uint16_t>(o_nc); q.mapq = O.at<uint8_t>(o_mq);
            q.l_read_name = O.at<uint8_t>(o_ln); q.name_off = O.at<uint64_t>(o_no); q.n_records = N;
            const uint32_t rgrid = (uint32_t)((N + 255) / 256);
            t = T.begin(K_PILEUP);
            hipLaunchKernelGGL(fl::blob_chain_kernel<true>, dim3((nch + 255) / 256), dim3(256), 0, ctx->stream, a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(fl::blob_record_kernel, dim3(rgrid), dim3(256), 0, ctx->stream, q);
            HIPCHK(hipGetLastError());
            launch_offset_scan(ctx, q.name_off, O.at<uint64_t>(o_tile), (uint32_t)N);
            HIPCHK(hipGetLastError());
            T.end(t);
            t = T.begin(K_D2H);
            HIPCHK(hipMemcpyAsync(&name_bytes, q.name_off + N, 8, hipMemcpyDeviceToHost, ctx->stream));
            T.end(t);
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (name_bytes > 255 * N) return fail(FLORIA_E_DEVICE, "blob_records: the names are longer than 255 bytes per record");
            if (int rc = ctx->rec_names.ensure(name_bytes + 256)) return rc;
            q.names = ctx->rec_names.as<uint8_t>();
            t = T.begin(K_PILEUP);
            hipLaunchKernelGGL(fl::blob_names_kernel, dim3(rgrid), dim3(256), 0, ctx->stream, q);
            HIPCHK(hipGetLastError());
            T.end(t);
        }
    }
    R->n_records = N;
    R->offset = (uint64_t*)cells_bytes(8 * N); R->block_size = (uint32_t*)cells_bytes(4 * N); R->ref_id = (int32_t*)cells_bytes(4 * N); R->pos = (int32_t*)cells_bytes(4 * N);
    R->l_seq = (uint32_t*)cells_bytes(4 * N); R->cigar0 = (uint32_t*)cells_bytes(4 * N); R->flag = (uint16_t*)cells_bytes(2 * N); R->n_cigar_op = (uint16_t*)cells_bytes(2 * N);
    R->mapq = (uint8_t*)cells_bytes(N); R->l_read_name = (uint8_t*)cells_bytes(N); R->name_off = (uint64_t*)cells_bytes(8 * (N + 1)); R->names = (uint8_t*)cells_bytes(name_bytes);
    if (!R->offset || !R->block_size || !R->ref_id || !R->pos || !R->l_seq || !R->cigar0 || !R->flag || !R->n_cigar_op || !R->mapq || !R->l_read_name || !R->name_off || !R->names)
        return fail(FLORIA_E_NOMEM, "malloc");
    R->name_off[0] = 0;
    if (N) {
        const int t = T.begin(K_D2H);
        const auto down = [&](void* dst, const void* src, uint64_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; };
        HIPCHK(down(R->offset, q.rec_off, 8 * N)); HIPCHK(down(R->block_size, q.block_size, 4 * N)); HIPCHK(down(R->ref_id, q.ref_id, 4 * N)); HIPCHK(down(R->pos, q.pos, 4 * N));
        HIPCHK(down(R->l_seq, q.l_seq, 4 * N)); HIPCHK(down(R->cigar0, q.cigar0, 4 * N)); HIPCHK(down(R->flag, q.flag, 2 * N)); HIPCHK(down(R->n_cigar_op, q.n_cigar_op, 2 * N));
        HIPCHK(down(R->mapq, q.mapq, N)); HIPCHK(down(R->l_read_name, q.l_read_name, N)); HIPCHK(down(R->name_off, q.name_off, 8 * (N + 1))); HIPCHK(down(R->names, q.names, name_bytes));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (nch) T.publish(ctx->timing);
    guard.r = nullptr;
    *out = R;
    return 0;
}

void floria_hip_blob_sequences_free(floria_blob_sequences* r) {
    if (!r) return;
    g_big.put(r->base_off); g_big.put(r->bases); g_big.put(r->quals);
    free(r);
}

int floria_hip_blob_sequences(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* seq_off, const uint32_t* l_seq, const uint64_t* qual_off, uint64_t n, floria_blob_sequences** out) {
    if (!ctx || !blob || !out || (n && (!seq_off || !l_seq || !qual_off))) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (blob->ctx != ctx) return fail(FLORIA_E_INVALID, "the blob belongs to another context");
    if (n >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "blob_sequences: 2^32 and more records");
    // the host part: every range against the blob's length, before anything is uploaded or launched
    const uint64_t B = blob->bytes;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t ls = l_seq[i], packed = (ls + 1) / 2;
        const char* what = seq_off[i] > B || packed > B - seq_off[i] ? "sequence" : qual_off[i] > B || ls > B - qual_off[i] ? "quality" : nullptr;
        if (what) return fail(FLORIA_E_INVALID, std::string("blob_sequences: the ") + what + " bytes of record " + std::to_string(i) + " reach past the blob (" + std::to_string(B) + " bytes)");
        total += ls;
    }
    if (total >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "blob_sequences: 2^32 and more bases (" + std::to_string(total) + ")");
    floria_blob_sequences* R = (floria_blob_sequences*)calloc(1, sizeof(floria_blob_sequences));
    if (!R) return fail(FLORIA_E_NOMEM, "calloc");
    struct Guard { floria_blob_sequences* r; hipStream_t st; ~Guard() { if (r) { (void)hipStreamSynchronize(st); floria_hip_blob_sequences_free(r); } } } guard{R, ctx->stream};
    R->n = n;
    R->base_off = (uint64_t*)cells_bytes(8 * (n + 1)); R->bases = (uint8_t*)cells_bytes(total); R->quals = (uint8_t*)cells_bytes(total);
    if (!R->base_off || !R->bases || !R->quals) return fail(FLORIA_E_NOMEM, "malloc");
    R->base_off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) R->base_off[i + 1] = R->base_off[i] + l_seq[i];
    ctx->timing = floria_timing{};
    if (total) {
        HIPCHK(hipSetDevice(ctx->device));
        Carve C, O;
        const Seg s_so = C.seg(8 * n), s_qo = C.seg(8 * n), s_ls = C.seg(4 * n), s_bo = C.seg(8 * (n + 1));
        const Seg o_b = O.seg(total), o_q = O.seg(total);
        if (int rc = C.place(ctx->seq_in)) return rc;
        if (int rc = O.place(ctx->seq_out)) return rc;
        EventTimer T(ctx->stream);
        int t = T.begin(K_H2D);
        HIPCHK(C.up(s_so, seq_off, 8 * n, ctx->stream)); HIPCHK(C.up(s_qo, qual_off, 8 * n, ctx->stream)); HIPCHK(C.up(s_ls, l_seq, 4 * n, ctx->stream));
        HIPCHK(C.up(s_bo, R->base_off, 8 * (n + 1), ctx->stream));
        T.end(t);
        fl::BlobSeqArgs a{};
        a.blob = blob->buf.as<const uint8_t>(); a.seq_off = C.at<const uint64_t>(s_so); a.qual_off = C.at<const uint64_t>(s_qo); a.l_seq = C.at<const uint32_t>(s_ls);
        a.base_off = C.at<const uint64_t>(s_bo); a.bases = O.at<uint8_t>(o_b); a.quals = O.at<uint8_t>(o_q); a.n = n;
        const uint64_t wgs = (n + fl::SEQ_WAVES - 1) / fl::SEQ_WAVES;
        t = T.begin(K_PILEUP);
        hipLaunchKernelGGL(fl::blob_seq_kernel, dim3((uint32_t)std::min<uint64_t>(wgs, 8ull * (uint64_t)ctx->n_cu)), dim3(64 * fl::SEQ_WAVES), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        T.end(t);
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(R->bases, a.bases, total, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(hipMemcpyAsync(R->quals, a.quals, total, hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        T.publish(ctx->timing);
    }
    guard.r = nullptr;
    *out = R;
    return 0;
}

void floria_hip_estimate_result_free(floria_estimate_result* r) {
    if (!r) return;
    g_big.put(r->col_group); g_big.put(r->col_pos); g_big.put(r->col_total); g_big.put(r->col_most); g_big.put(r->rec_hits);
    free(r);
}

// The -e / -l estimate on a blob (estimate_kernel.h).  The host part checks every range, runs the span pass, then walks each group in position windows that hold
// covered positions only at their start (a gap between records is jumped, never scanned) and reads the chain's state back after every window: the number of sampled
// columns sizes the count pass, `done` ends the walk.
int floria_hip_blob_estimate(floria_hip_ctx* ctx, const floria_hip_blob* blob, const floria_estimate_records* E, uint32_t stop, floria_estimate_state* inout, floria_estimate_result** out) {
    if (!ctx || !blob || !E || !inout || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    const uint64_t n = E->n;
    if ((n && (!E->pos || !E->cigar_off || !E->n_cigar || !E->seq_off || !E->l_seq)) || !E->group_off) return fail(FLORIA_E_INVALID, "null argument");
    if (blob->ctx != ctx) return fail(FLORIA_E_INVALID, "the blob belongs to another context");
    if (n >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "blob_estimate: 2^32 and more records");
    // the host part: the groups, every position and every range against the blob's length, before anything is uploaded or launched
    const uint32_t ng = E->n_groups;
    if (E->group_off[0] != 0) return fail(FLORIA_E_INVALID, "blob_estimate: group_off does not start at 0");
    for (uint32_t g = 0; g < ng; ++g)
        if (E->group_off[g] > E->group_off[g + 1]) return fail(FLORIA_E_INVALID, "blob_estimate: group_off descends at group " + std::to_string(g));
    if (E->group_off[ng] != n) return fail(FLORIA_E_INVALID, "blob_estimate: group_off ends at " + std::to_string(E->group_off[ng]) + ", not at the " + std::to_string(n) + " records");
    const uint64_t B = blob->bytes;
    for (uint32_t g = 0; g < ng; ++g)
        for (uint64_t i = E->group_off[g]; i < E->group_off[g + 1]; ++i) {
            const std::string rec = "blob_estimate: record " + std::to_string(i);
            if (E->n_cigar[i] == 0) return fail(FLORIA_E_INVALID, rec + " has no CIGAR operation");
            if (E->pos[i] < 0) return fail(FLORIA_E_INVALID, rec + " has a negative pos (" + std::to_string(E->pos[i]) + ")");
            if (i > E->group_off[g] && E->pos[i] < E->pos[i - 1]) return fail(FLORIA_E_INVALID, rec + ": pos descends inside group " + std::to_string(g));
            const uint64_t cig = 4ull * E->n_cigar[i], packed = ((uint64_t)E->l_seq[i] + 1) / 2;
            const char* what = E->cigar_off[i] > B || cig > B - E->cigar_off[i] ? "CIGAR" : E->seq_off[i] > B || packed > B - E->seq_off[i] ? "sequence" : nullptr;
            if (what) return fail(FLORIA_E_INVALID, "blob_estimate: the " + std::string(what) + " bytes of record " + std::to_string(i) + " reach past the blob (" + std::to_string(B) + " bytes)");
        }
    floria_estimate_result* R = (floria_estimate_result*)calloc(1, sizeof(floria_estimate_result));
    if (!R) return fail(FLORIA_E_NOMEM, "calloc");
    struct Guard { floria_estimate_result* r; hipStream_t st; ~Guard() { if (r) { (void)hipStreamSynchronize(st); floria_hip_estimate_result_free(r); } } } guard{R, ctx->stream};
    R->rec_hits = (uint32_t*)cells_bytes(4 * n);
    if (!R->rec_hits) return fail(FLORIA_E_NOMEM, "malloc");
    memset(R->rec_hits, 0, 4 * n);
    ctx->timing = floria_timing{};
    std::vector<uint32_t> col_group, col_total, col_most;
    std::vector<int32_t> col_pos;
    auto finish = [&]() -> int {
        const size_t nc = col_group.size();
        R->n_cols = nc;
        R->col_group = (uint32_t*)cells_bytes(4 * nc); R->col_pos = (int32_t*)cells_bytes(4 * nc); R->col_total = (uint32_t*)cells_bytes(4 * nc); R->col_most = (uint32_t*)cells_bytes(4 * nc);
        if (!R->col_group || !R->col_pos || !R->col_total || !R->col_most) return fail(FLORIA_E_NOMEM, "malloc");
        if (nc) { memcpy(R->col_group, col_group.data(), 4 * nc); memcpy(R->col_pos, col_pos.data(), 4 * nc); memcpy(R->col_total, col_total.data(), 4 * nc); memcpy(R->col_most, col_most.data(), 4 * nc); }
        guard.r = nullptr;
        *out = R;
        return 0;
    };
    if (inout->n_err >= stop) { R->done = 1; return finish(); }
    if (n == 0) return finish();

    HIPCHK(hipSetDevice(ctx->device));
    EventTimer T(ctx->stream);
    Carve C;
    const Seg s_pos = C.seg(4 * n), s_co = C.seg(8 * n), s_nc = C.seg(4 * n), s_so = C.seg(8 * n), s_ls = C.seg(4 * n), s_end = C.seg(8 * n), s_hits = C.seg(4 * n);
    if (int rc = C.place(ctx->est_in)) return rc;
    int t = T.begin(K_H2D);
    HIPCHK(C.up(s_pos, E->pos, 4 * n, ctx->stream)); HIPCHK(C.up(s_co, E->cigar_off, 8 * n, ctx->stream)); HIPCHK(C.up(s_nc, E->n_cigar, 4 * n, ctx->stream));
    HIPCHK(C.up(s_so, E->seq_off, 8 * n, ctx->stream)); HIPCHK(C.up(s_ls, E->l_seq, 4 * n, ctx->stream));
    HIPCHK(hipMemsetAsync(C.at<>(s_hits), 0, 4 * n, ctx->stream));
    T.end(t);
    fl::EstRecs recs{};
    recs.blob = blob->buf.as<const uint8_t>(); recs.pos = C.at<const int32_t>(s_pos); recs.cigar_off = C.at<const uint64_t>(s_co); recs.n_cigar = C.at<const uint32_t>(s_nc);
    recs.seq_off = C.at<const uint64_t>(s_so); recs.l_seq = C.at<const uint32_t>(s_ls); recs.end = C.at<int64_t>(s_end); recs.rec_hits = C.at<uint32_t>(s_hits);
    const uint32_t max_wgs = 8u * (uint32_t)ctx->n_cu;
    auto rec_grid = [&](uint64_t recs_n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((recs_n + fl::EST_WAVES - 1) / fl::EST_WAVES, max_wgs))); };
    t = T.begin(K_PILEUP);
    hipLaunchKernelGGL(fl::est_span_kernel, rec_grid(n), dim3(64 * fl::EST_WAVES), 0, ctx->stream, recs, n);
    HIPCHK(hipGetLastError());
    T.end(t);
    std::vector<int64_t> end(n);
    t = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(end.data(), recs.end, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    T.end(t);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int64_t widest = 1;
    for (uint32_t g = 0; g < ng; ++g) {
        int64_t top = 0;
        for (uint64_t i = E->group_off[g]; i < E->group_off[g + 1]; ++i) {
            if (end[i] > (int64_t)0x7fffffff) return fail(FLORIA_E_UNSUPPORTED, "blob_estimate: record " + std::to_string(i) + " ends at " + std::to_string(end[i]) + ", beyond 2^31 - 1");
            top = std::max(top, end[i]);
        }
        if (E->group_off[g] < E->group_off[g + 1]) widest = std::max(widest, top - (int64_t)E->pos[E->group_off[g]]);
    }
    // one window's arrays, sized for the widest window any group needs
    const uint32_t win = (uint32_t)std::min<int64_t>(ctx->estimate_window ? ctx->estimate_window : (1u << 22), widest);
    const uint32_t max_chunks = (win + fl::EST_CHUNK - 1) / fl::EST_CHUNK;
    const size_t padded = (size_t)max_chunks * fl::EST_CHUNK;
    const uint32_t max_iv = (uint32_t)std::min<uint64_t>((uint64_t)(stop - inout->n_err) + 1, (uint64_t)win / fl::EST_PERIOD + 2);      // starts lie 1000 ordinals apart; all but the last reach a deep column
    Carve Wc;
    const Seg w_ord = Wc.seg(4 * padded), w_tot = Wc.seg(4 * padded), w_poo = Wc.seg(4 * padded), w_nd = Wc.seg(4 * padded);
    const Seg w_sc = Wc.seg(4 * (size_t)max_chunks), w_sd = Wc.seg(4 * (size_t)max_chunks), w_nc = Wc.seg(4 * (size_t)max_chunks), w_fd = Wc.seg(4 * (size_t)max_chunks);
    const Seg w_iv = Wc.seg(12 * (size_t)max_iv), w_st = Wc.seg(sizeof(fl::EstState));
    if (int rc = Wc.place(ctx->est_win)) return rc;
    fl::EstWindow W{};
    W.ord = Wc.at<uint32_t>(w_ord); W.tot = Wc.at<uint32_t>(w_tot); W.pos_of_ord = Wc.at<uint32_t>(w_poo); W.next_deep = Wc.at<uint32_t>(w_nd);
    W.sum_cov = Wc.at<int32_t>(w_sc); W.sum_dep = Wc.at<int32_t>(w_sd); W.n_cov = Wc.at<int32_t>(w_nc); W.first_deep = Wc.at<uint32_t>(w_fd);
    uint32_t* const d_iv = Wc.at<uint32_t>(w_iv);
    fl::EstState* const d_st = Wc.at<fl::EstState>(w_st);
    fl::EstState st{};
    st.count = inout->count; st.n_err = inout->n_err;
    t = T.begin(K_H2D);
    HIPCHK(hipMemcpyAsync(d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    T.end(t);

    for (uint32_t g = 0; g < ng && !st.done; ++g) {
        const uint64_t g0 = E->group_off[g], g1 = E->group_off[g + 1];
        if (g0 == g1) continue;
        uint64_t lo = g0, hi = g0;                     // records [lo, hi) may meet the window: everything in front of lo ends before it, everything from hi on begins behind it
        int64_t w0 = E->pos[g0];
        while (!st.done) {
            const int64_t w1 = w0 + (int64_t)win;
            while (lo < g1 && end[lo] <= w0) ++lo;
            while (hi < g1 && (int64_t)E->pos[hi] < w1) ++hi;
            W.w0 = w0; W.wn = win; W.n_chunks = max_chunks;
            const dim3 chunks(std::min<uint32_t>(max_chunks, max_wgs)), threads(fl::EST_THREADS);
            t = T.begin(K_PILEUP);
            HIPCHK(hipMemsetAsync(W.ord, 0, 4 * padded, ctx->stream)); HIPCHK(hipMemsetAsync(W.tot, 0, 4 * padded, ctx->stream));
            hipLaunchKernelGGL(fl::est_mark_kernel, rec_grid(hi - lo), dim3(64 * fl::EST_WAVES), 0, ctx->stream, recs, lo, hi, W);
            hipLaunchKernelGGL(fl::est_sum_kernel, chunks, threads, 0, ctx->stream, W);
            hipLaunchKernelGGL(fl::est_tables_kernel, dim3(1), threads, 0, ctx->stream, W.sum_cov, W.sum_dep, (uint32_t*)nullptr, max_chunks, (uint32_t*)nullptr);
            hipLaunchKernelGGL(fl::est_depth_kernel, chunks, threads, 0, ctx->stream, W);
            hipLaunchKernelGGL(fl::est_tables_kernel, dim3(1), threads, 0, ctx->stream, W.n_cov, (int32_t*)nullptr, W.first_deep, max_chunks, &d_st->n_cov);
            hipLaunchKernelGGL(fl::est_ordinal_kernel, chunks, threads, 0, ctx->stream, W);
            hipLaunchKernelGGL(fl::est_chain_kernel, dim3(1), dim3(64), 0, ctx->stream, d_st, stop, W, d_iv, max_iv);
            HIPCHK(hipGetLastError());
            T.end(t);
            t = T.begin(K_D2H);
            HIPCHK(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
            T.end(t);
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (st.overflow) return fail(FLORIA_E_DEVICE, "blob_estimate: the hop chain met more intervals than its list holds (" + std::to_string(max_iv) + ")");
            if (st.n_cols) {
                const uint32_t nc = st.n_cols;
                Carve Cc;
                const Seg c_pos = Cc.seg(4 * (size_t)nc), c_cnt = Cc.seg(64 * (size_t)nc), c_tot = Cc.seg(4 * (size_t)nc), c_most = Cc.seg(4 * (size_t)nc);
                if (int rc = Cc.place(ctx->est_cols)) return rc;
                t = T.begin(K_PILEUP);
                HIPCHK(hipMemsetAsync(Cc.at<>(c_cnt), 0, 64 * (size_t)nc, ctx->stream));
                hipLaunchKernelGGL(fl::est_expand_kernel, dim3(std::min<uint32_t>(std::min(st.n_iv, max_iv), max_wgs)), threads, 0, ctx->stream, d_iv, std::min(st.n_iv, max_iv), W.pos_of_ord, Cc.at<uint32_t>(c_pos));
                hipLaunchKernelGGL(fl::est_count_kernel, rec_grid(hi - lo), dim3(64 * fl::EST_WAVES), 0, ctx->stream, recs, lo, hi, w0, win, Cc.at<const uint32_t>(c_pos), nc, Cc.at<uint32_t>(c_cnt));
                hipLaunchKernelGGL(fl::est_reduce_kernel, dim3(std::min<uint32_t>((nc + fl::EST_THREADS - 1) / fl::EST_THREADS, max_wgs)), threads, 0, ctx->stream, Cc.at<const uint32_t>(c_cnt), nc,
                                   Cc.at<uint32_t>(c_tot), Cc.at<uint32_t>(c_most));
                HIPCHK(hipGetLastError());
                T.end(t);
                const size_t at = col_group.size();
                col_group.resize(at + nc, g); col_pos.resize(at + nc); col_total.resize(at + nc); col_most.resize(at + nc);
                t = T.begin(K_D2H);
                HIPCHK(hipMemcpyAsync(col_pos.data() + at, Cc.at<>(c_pos), 4 * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(hipMemcpyAsync(col_total.data() + at, Cc.at<>(c_tot), 4 * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(hipMemcpyAsync(col_most.data() + at, Cc.at<>(c_most), 4 * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
                T.end(t);
                HIPCHK(hipStreamSynchronize(ctx->stream));
                for (size_t i = at; i < at + nc; ++i) col_pos[i] = (int32_t)(w0 + col_pos[i]);      // (the window's relative positions; every end is <= 2^31 - 1)
            }
            // the next window: right behind this one while a record reaches over its end, else at the next record
            while (lo < hi && end[lo] <= w1) ++lo;
            if (lo < hi) w0 = w1;
            else if (hi < g1) w0 = E->pos[hi];
            else break;
        }
    }
    t = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(R->rec_hits, recs.rec_hits, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    T.end(t);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    T.publish(ctx->timing);
    inout->count = st.count; inout->n_err = st.n_err;
    R->done = st.done;
    return finish();
}

int floria_hip_pileup_records_resident_blob(floria_hip_ctx* ctx, const floria_hip_blob* blob, const floria_alignments* A, const floria_snp_table* S, const floria_ref_seqs* F,
                                            const floria_realign_walk* walk, floria_record_summary** out) {
    if (!out || !blob) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    floria_record_summary* Y = (floria_record_summary*)calloc(1, sizeof(floria_record_summary));
    if (!Y) return fail(FLORIA_E_NOMEM, "calloc");
    floria_record_cells* R = nullptr;
    if (int rc = pileup_records_impl(ctx, A, S, F, walk, &R, &Y->counts, true, blob)) { free(Y); return rc; }
    Y->n_records = R->n_records; Y->cell_off = R->cell_off; Y->first_snp = R->snp; Y->last_snp = R->seq_pos; Y->ref_end = R->ref_end;
    free(R);
    Y->token = ++ctx->token_counter;
    ctx->res_token = Y->token; ctx->res_summary = Y;
    *out = Y;
    return 0;
}

// `ordered`: floria_hip_assemble_contigs_ordered — the contigs that hold a merged fragment get their set_order from the device (assemble_order_kernel.h)
// `keep_sp`: floria_hip_assemble_contigs_opt with FLORIA_ASM_KEEP_SEQ_POS — every contig carries the SEQ_POS words of its cells; part_mate [n_parts] or null
static int assemble_impl(floria_hip_ctx* ctx, const floria_record_summary* Y, const floria_fragment_plan* plan, floria_hip_contig** out, bool ordered, bool keep_sp = false,
                         const uint8_t* part_mate = nullptr) {
    if (!ctx || !Y || !plan || !out || !plan->frag_off) return fail(FLORIA_E_INVALID, "null argument");
    const uint32_t nc = plan->n_contigs;
    for (uint32_t c = 0; c < nc; ++c) out[c] = nullptr;
    if (ordered && plan->set_order) return fail(FLORIA_E_INVALID, "assemble: the plan gives a set_order and the call is asked to derive it (give the order or ask for it, not both)");
    if (!ctx->res_token || Y != ctx->res_summary || Y->token != ctx->res_token)
        return fail(FLORIA_E_INVALID, "assemble: the record summary is not the context's live residency (a later floria_hip_pileup_records* call has replaced its cells)");
    if (nc != ctx->res_n_contigs) return fail(FLORIA_E_INVALID, "assemble: the plan has " + std::to_string(nc) + " contigs, the resident pileup's SNP table has " + std::to_string(ctx->res_n_contigs));
    if (nc == 0) return 0;
    // ---- everything the host can check from the summary, before anything is launched ----
    const uint32_t n_rec = Y->n_records;
    if (plan->frag_off[0] != 0) return fail(FLORIA_E_INVALID, "assemble: frag_off does not start at 0");
    for (uint32_t c = 0; c < nc; ++c) {
        if (plan->frag_off[c + 1] < plan->frag_off[c]) return fail(FLORIA_E_INVALID, "assemble: frag_off decreases at contig " + std::to_string(c));
        if (plan->frag_off[c + 1] - plan->frag_off[c] >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "more than 2^32 fragments in one contig");
    }
    const uint64_t NF = plan->frag_off[nc];
    if (NF >= (1ull << 32) - fl::PILEUP_SCAN_TILE) return fail(FLORIA_E_UNSUPPORTED, "assemble: 2^32 and more fragments in one call");
    if (NF && (!plan->part_off || !plan->part_rec)) return fail(FLORIA_E_INVALID, "null argument");
    if (NF && plan->part_off[0] != 0) return fail(FLORIA_E_INVALID, "assemble: part_off does not start at 0");
    std::vector<uint32_t> frag_ctg((size_t)NF);
    std::vector<uint32_t> merged(ordered ? nc : 0, 0);      // ordered: != 0 for a contig with a fragment of two or more parts that have cells
    std::vector<uint64_t> part_cells(ordered ? (size_t)NF : 0);      // ... and the cells of every fragment's parts together
    for (uint32_t c = 0; c < nc; ++c)
        for (uint64_t f = plan->frag_off[c]; f < plan->frag_off[c + 1]; ++f) {
            frag_ctg[f] = c;
            const uint64_t p0 = plan->part_off[f], p1 = plan->part_off[f + 1];
            const auto where = [&]() { return "fragment " + std::to_string((unsigned long long)(f - plan->frag_off[c])) + " of contig " + std::to_string(c); };
            if (p1 < p0) return fail(FLORIA_E_INVALID, "assemble: part_off decreases at " + where());
            if (p1 == p0) return fail(FLORIA_E_INVALID, "assemble: " + where() + " has no part");
            bool any = false;
            uint64_t with = 0, sum = 0;
            for (uint64_t p = p0; p < p1; ++p) {
                const uint32_t rec = plan->part_rec[p];
                if (rec >= n_rec) return fail(FLORIA_E_INVALID, "assemble: " + where() + " names record " + std::to_string(rec) + " of " + std::to_string(n_rec));
                if (ctx->res_contig[rec] != c) return fail(FLORIA_E_INVALID, "assemble: record " + std::to_string(rec) + " lies on contig " + std::to_string(ctx->res_contig[rec]) + ", " + where() + " does not");
                any = any || Y->cell_off[rec + 1] > Y->cell_off[rec];
                if (Y->cell_off[rec + 1] > Y->cell_off[rec]) { ++with; sum += Y->cell_off[rec + 1] - Y->cell_off[rec]; }
            }
            if (ordered) { part_cells[f] = sum; if (with >= 2) merged[c] = 1; }
            if (!any) return fail(FLORIA_E_INVALID, "assemble: the parts of " + where() + " have no cell (every read has >= 1 cell)");
        }
    const uint64_t NP = NF ? plan->part_off[NF] : 0;
    if (part_mate) for (uint64_t p = 0; p < NP; ++p) if (part_mate[p] > 1) return fail(FLORIA_E_INVALID, "assemble: part_mate of part " + std::to_string((unsigned long long)p) + " is " + std::to_string((unsigned)part_mate[p]) + " (0 or 1)");
    // ordered: what the general kernel may meet — the fragments beyond the wavefront kernel's tables and the largest of them (the scratch is sized before any launch)
    bool any_merged = false;
    uint64_t n_general = 0, cells_max = 0;
    if (ordered)
        for (uint32_t c = 0; c < nc; ++c) {
            if (!merged[c]) continue;
            any_merged = true;
            for (uint64_t f = plan->frag_off[c]; f < plan->frag_off[c + 1]; ++f)
                if (part_cells[f] > fl::AO_FAST_CELLS || ctx->knobs.asm_order_general) { ++n_general; cells_max = std::max(cells_max, part_cells[f]); }
        }
    if (cells_max >= (1ull << 31)) return fail(FLORIA_E_UNSUPPORTED, "assemble: a fragment whose parts have 2^31 and more cells");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = nc, nf32 = (uint32_t)NF;
    const uint32_t n_tiles = (nf32 + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
    // ---- the plan goes up; COUNT, offset scan, the per-contig cell totals come back (the only round trip: the arena is sized from them) ----
    Carve C;
    const Seg s_po = C.seg(8 * (NF + 1)), s_pr = C.seg(4 * NP + 4), s_fc = C.seg(4 * NF + 4), s_fo = C.seg(8ull * (n + 1)), s_cnt = C.seg(8 * (NF + 1)), s_tile = C.seg(8ull * n_tiles + 8),
              s_tot = C.seg(8ull * (n + 1)), s_cdev = C.seg(sizeof(fl::ContigDev) * n);
    const Seg s_mg = C.seg(any_merged ? 4ull * n : 0), s_todo = C.seg(any_merged ? 8 * (NF + 1) : 0);
    const Seg s_pm = C.seg(keep_sp && part_mate ? NP + 16 : 0), s_spf = C.seg(keep_sp ? 16 : 0);
    if (int rc = C.place(ctx->asm_plan)) return rc;
    fl::AsmOrderArgs oa{};
    if (n_general) {
        oa.cells_max = (uint32_t)cells_max; oa.ctrl_bytes = fl::fx_ctrl_bytes(oa.cells_max + 1); oa.slot_bytes = fl::fx_slot_bytes(oa.cells_max + 1);
        const uint64_t per = fl::AO_TABLES * (oa.ctrl_bytes + oa.slot_bytes);      // a thread's five tables; as many threads as 2 GiB hold, one at the least
        oa.n_threads = chain_grid(ctx, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_general, 65536), (2ull << 30) / per)));
        oa.scratch_bytes = per * oa.n_threads;
        if (int rc = ctx->asm_ord_scr.ensure(oa.scratch_bytes)) return rc;
        oa.scratch = ctx->asm_ord_scr.as<uint8_t>();
    }
    EventTimer T(ctx->stream);
    ctx->timing = floria_timing{};
    fl::AssembleArgs a{};
    a.cell_off = ctx->res_cell_off; a.snp = ctx->res_snp; a.allele = ctx->res_allele; a.qual = ctx->res_qual;
    a.part_off = C.at<const uint64_t>(s_po); a.part_rec = C.at<const uint32_t>(s_pr); a.frag_ctg = C.at<const uint32_t>(s_fc); a.frag_off = C.at<const uint64_t>(s_fo);
    a.frag_cells = C.at<uint64_t>(s_cnt); a.n_frags = NF;
    std::vector<uint64_t> cp(n + 1, 0);
    const uint32_t grid = items_grid(ctx, NF, 4);      // one wavefront per fragment
    int t = T.begin(K_H2D);
    if (NF) { HIPCHK(C.up(s_po, plan->part_off, 8 * (NF + 1), ctx->stream)); HIPCHK(C.up(s_pr, plan->part_rec, 4 * NP, ctx->stream)); HIPCHK(C.up(s_fc, frag_ctg.data(), 4 * NF, ctx->stream)); }
    HIPCHK(C.up(s_fo, plan->frag_off, 8ull * (n + 1), ctx->stream));
    T.end(t);
    if (NF) {
        t = T.begin(K_PILEUP);
        hipLaunchKernelGGL((fl::assemble_kernel<false, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        launch_offset_scan(ctx, a.frag_cells, C.at<uint64_t>(s_tile), nf32);
        hipLaunchKernelGGL(fl::assemble_totals_kernel, dim3((n + 256) / 256), dim3(256), 0, ctx->stream, (const uint64_t*)a.frag_cells, a.frag_off, C.at<uint64_t>(s_tot), n + 1);
        HIPCHK(hipGetLastError());
        T.end(t);
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(cp.data(), C.at(s_tot), 8ull * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n; ++i) {
        if (cp[i + 1] < cp[i]) return fail(FLORIA_E_DEVICE, "assemble: the cell offsets do not ascend");
        if (cp[i + 1] - cp[i] >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "more than 2^32 cells in one contig");
    }
    // ---- the arena, as an upload of a CSR batch of these sizes would have it ----
    std::vector<uint64_t> rp(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) rp[i + 1] = plan->frag_off[i + 1];
    const uint64_t CC = cp[n];
    const bool derive_so = any_merged && CC != 0;
    const bool any_so = (plan->set_order != nullptr && CC != 0) || derive_so;
    UploadPlan P;
    if (int rc = P.open(ctx, n, std::move(rp), std::move(cp), any_so, keep_sp, out, true)) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (keep_sp) P.sp_dev[i] = P.sp_at(i);
        if (any_so && P.ucd[i].n_reads && (!derive_so || merged[i])) P.so_dev[i] = P.so_at(i);
    }
    char *D = P.D, *so_all = D + P.Y.o_so;
    // ---- FILL writes the raw CSR arrays where an upload's DMA would have put them; then the upload's own validate + flatten launch ----
    a.read_off = (uint32_t*)(D + P.Y.o_ro); a.first = (uint32_t*)(D + P.Y.o_first); a.last = (uint32_t*)(D + P.Y.o_last);
    a.out_snp = (uint32_t*)(D + P.Y.o_snp); a.out_allele = (uint8_t*)(P.T + P.t_al); a.out_qual = (uint8_t*)(P.T + P.t_q);
    if (keep_sp) { a.seq_pos = ctx->res_seq_pos; a.part_mate = part_mate ? C.at<const uint8_t>(s_pm) : nullptr; a.out_sp = (uint32_t*)(D + P.Y.o_sp); a.sp_overflow = C.at<uint32_t>(s_spf); }
    uint32_t sp_overflow = 0;
    uint64_t pinned_b = 0, staged_b = 0;
    t = T.begin(K_H2D);
    if (any_so && !derive_so) { std::vector<CopyRun> runs{{(const char*)plan->set_order, so_all, (size_t)(4 * CC)}}; if (int rc = issue_copies(ctx, runs, &pinned_b, &staged_b)) return rc; }
    if (derive_so) HIPCHK_AS("assemble: ", C.up(s_mg, merged.data(), 4ull * n, ctx->stream));
    HIPCHK_AS("assemble: ", issue_tables(ctx, P, ctx->stream));
    if (keep_sp) { HIPCHK_AS("assemble: ", hipMemsetAsync(C.at(s_spf), 0, 16, ctx->stream)); if (part_mate) HIPCHK_AS("assemble: ", C.up(s_pm, part_mate, NP, ctx->stream)); }
    T.end(t);
    if (NF) {
        t = T.begin(K_PILEUP);
        if (keep_sp) hipLaunchKernelGGL((fl::assemble_kernel<true, true>), dim3(grid), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((fl::assemble_kernel<true, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
        HIPCHK_AS("assemble: ", hipGetLastError());
        if (derive_so) {
            // the set orders of the merged contigs' fragments, where an uploaded set_order would lie.  Preset to all ones: whatever the kernels leave unwritten
            // is no permutation, and the cell orders below refuse it.
            oa.cell_off = a.cell_off; oa.snp = a.snp; oa.part_off = a.part_off; oa.part_rec = a.part_rec; oa.frag_ctg = a.frag_ctg; oa.frag_cells = a.frag_cells;
            oa.merged_snp = a.out_snp; oa.ctg_merged = C.at<const uint32_t>(s_mg); oa.set_order = (uint32_t*)so_all; oa.todo = C.at<uint64_t>(s_todo);
            oa.n_frags = NF; oa.n_parts = NP; oa.total_cells = CC; oa.n_records = n_rec; oa.n_contigs = n; oa.force_general = ctx->knobs.asm_order_general;
            HIPCHK_AS("assemble: ", hipMemsetAsync(so_all, 0xff, 4 * CC, ctx->stream));
            HIPCHK_AS("assemble: ", hipMemsetAsync(oa.todo, 0, 8, ctx->stream));
            hipLaunchKernelGGL(fl::assemble_order_kernel, dim3(grid), dim3(256), 0, ctx->stream, oa);
            HIPCHK_AS("assemble: ", hipGetLastError());
            if (n_general) {
                hipLaunchKernelGGL(fl::assemble_order_general_kernel, dim3((oa.n_threads + 63) / 64), dim3(64), 0, ctx->stream, oa);
                HIPCHK_AS("assemble: ", hipGetLastError());
            }
        }
        T.end(t);
    }
    t = T.begin(K_SEL);
    HIPCHK_AS("assemble: ", launch_flatten(ctx, P, 0, ctx->stream));
    T.end(t);
    t = T.begin(K_D2H);
    HIPCHK_AS("assemble: ", hipMemcpyAsync(P.ust.data(), P.T + P.t_st, sizeof(fl::UploadStatus) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (keep_sp) HIPCHK_AS("assemble: ", hipMemcpyAsync(&sp_overflow, C.at(s_spf), 4, hipMemcpyDeviceToHost, ctx->stream));
    T.end(t);
    HIPCHK_AS("assemble: ", hipStreamSynchronize(ctx->stream));
    if (sp_overflow) return fail(FLORIA_E_UNSUPPORTED, "assemble: a sequence position of 2^31 and more cannot be kept (the SEQ_POS word has 31 bits for it)");
    if (int rc = P.commit()) return rc;
    if (any_so) {                                          // the cell orders of the batch, now: a set_order that is no permutation is refused here, and "arith" = 1 reuses them
        std::vector<fl::ContigDev> cdev(n); std::vector<uint64_t> ncells(n); uint32_t len_max = 1;
        for (uint32_t i = 0; i < n; ++i) { cdev[i] = out[i]->dev; ncells[i] = out[i]->n_cells; len_max = std::max(len_max, out[i]->max_len); }
        // (the handles own the arena by now: until the orders stand, an error return frees them, behind the device)
        struct Handles { floria_hip_ctx* ctx; floria_hip_contig** h; uint32_t n; ~Handles() { if (h) { sync_all(ctx); for (uint32_t c = 0; c < n; ++c) { floria_hip_contig_free(h[c]); h[c] = nullptr; } } } } own{ctx, out, nc};
        HIPCHK_AS("assemble: ", hipMemcpyAsync(C.at(s_cdev), cdev.data(), sizeof(fl::ContigDev) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK_AS("assemble: ", hipStreamSynchronize(ctx->stream));
        if (int rc = cell_orders(ctx, C.at<const fl::ContigDev>(s_cdev), cdev, ncells, len_max)) return rc;
        own.h = nullptr;
    }
    T.publish(ctx->timing);
    ctx->timing.upload_pinned_bytes = pinned_b; ctx->timing.upload_staged_bytes = staged_b;
    return 0;
}

int floria_hip_assemble_contigs(floria_hip_ctx* ctx, const floria_record_summary* Y, const floria_fragment_plan* plan, floria_hip_contig** out) {
    return assemble_impl(ctx, Y, plan, out, false);
}

int floria_hip_assemble_contigs_ordered(floria_hip_ctx* ctx, const floria_record_summary* Y, const floria_fragment_plan* plan, floria_hip_contig** out) {
    return assemble_impl(ctx, Y, plan, out, true);
}

int floria_hip_assemble_contigs_opt(floria_hip_ctx* ctx, const floria_record_summary* Y, const floria_fragment_plan* plan, const floria_assemble_options* opts, floria_hip_contig** out) {
    if (out && plan) for (uint32_t c = 0; c < plan->n_contigs; ++c) out[c] = nullptr;
    if (!opts) return fail(FLORIA_E_INVALID, "null argument");
    if (opts->flags & ~(FLORIA_ASM_DERIVE_SET_ORDER | FLORIA_ASM_KEEP_SEQ_POS)) return fail(FLORIA_E_INVALID, "assemble: unknown flag bits " + std::to_string(opts->flags));
    const bool keep = (opts->flags & FLORIA_ASM_KEEP_SEQ_POS) != 0;
    if (opts->part_mate && !keep) return fail(FLORIA_E_INVALID, "assemble: part_mate is given without FLORIA_ASM_KEEP_SEQ_POS");
    return assemble_impl(ctx, Y, plan, out, (opts->flags & FLORIA_ASM_DERIVE_SET_ORDER) != 0, keep, opts->part_mate);
}

// ---- remove_monomorphic_allele (utils_frags.rs:713-772) on resident contigs (mono_kernel.h) ----------------------------------------------------------------------
int floria_hip_mono_timing(const floria_hip_ctx* ctx, double* ms6) {
    if (!ctx || !ms6) return fail(FLORIA_E_INVALID, "null argument");
    for (int k = 0; k < 6; ++k) ms6[k] = ctx->mono_ms[k];
    return 0;
}

void floria_hip_mono_result_free(floria_mono_result* r) {
    if (!r) return;
    free(r->read_off); free(r->old_read); free(r->removed); free(r->new_first); free(r->new_last); free(r);
}

int floria_hip_drop_monomorphic(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n, const uint64_t* snp_off, double error, int with_set_order,
                                floria_hip_contig** out, floria_mono_result** res) {
    if (res) *res = nullptr;
    if (out) for (uint32_t c = 0; c < n; ++c) out[c] = nullptr;
    if (!ctx || !out || !snp_off || (n && !contigs)) return fail(FLORIA_E_INVALID, "null argument");
    // ---- everything the host can tell, before anything is launched ----
    for (uint32_t c = 0; c < n; ++c) {
        if (!contigs[c]) return fail(FLORIA_E_INVALID, "null argument");
        if (contigs[c]->ctx != ctx) return fail(FLORIA_E_INVALID, "drop_monomorphic: contig " + std::to_string(c) + " belongs to another context");
    }
    if (snp_off[0] != 0) return fail(FLORIA_E_INVALID, "drop_monomorphic: snp_off does not start at 0");
    for (uint32_t c = 0; c < n; ++c) if (snp_off[c + 1] < snp_off[c]) return fail(FLORIA_E_INVALID, "drop_monomorphic: snp_off decreases at contig " + std::to_string(c));
    if (!std::isfinite(error)) return fail(FLORIA_E_INVALID, "drop_monomorphic: error is not finite");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint64_t> rp(n + 1, 0), cpi(n + 1, 0);          // input reads / cells before contig c
    for (uint32_t c = 0; c < n; ++c) {
        const floria_hip_contig* k = contigs[c];
        if (int rc = host_meta(k)) return rc;
        uint32_t hi = 0;
        for (uint32_t r = 0; r < k->n_reads; ++r) hi = std::max(hi, k->h_last[r]);
        if ((uint64_t)hi > snp_off[c + 1] - snp_off[c])
            return fail(FLORIA_E_INVALID, "drop_monomorphic: contig " + std::to_string(c) + " has a read that ends at SNP " + std::to_string(hi) + ", its SNP count is " + std::to_string((unsigned long long)(snp_off[c + 1] - snp_off[c])));
        rp[c + 1] = rp[c] + k->n_reads; cpi[c + 1] = cpi[c] + k->n_cells;
    }
    const uint64_t Rin = rp[n], S = snp_off[n];
    // (allocated behind the last launch; an error return releases it — after the arena's owner below has waited for the copies into it)
    struct Result { floria_mono_result* r = nullptr; ~Result() { floria_hip_mono_result_free(r); } } result;
    floria_mono_result*& M = result.r;
    const auto new_result = [&](uint64_t n_out, uint64_t n_mask) {
        M = (floria_mono_result*)calloc(1, sizeof(floria_mono_result));
        if (!M) return false;
        M->n_contigs = n;
        M->read_off = (uint64_t*)calloc(n + 1, 8); M->old_read = (uint32_t*)calloc(n_out + 1, 4); M->removed = (uint8_t*)calloc(n_mask + 1, 1);
        M->new_first = (uint32_t*)calloc(n_out + 1, 4); M->new_last = (uint32_t*)calloc(n_out + 1, 4);
        return M->read_off && M->old_read && M->removed && M->new_first && M->new_last;
    };
    if (n == 0) {
        if (res) { if (!new_result(0, 0)) return fail(FLORIA_E_NOMEM, "calloc"); *res = M; M = nullptr; }
        return 0;
    }
    EventTimer T(ctx->stream);
    ctx->timing = floria_timing{};
    enum { K_CLEAR = 20, K_COUNT = 21, K_DECIDE = 22, K_FCOUNT = 23, K_FILL = 24, K_ORDER = 25 };      // (the device work of pileup_ms, one kind each: floria_hip_mono_timing)
    // ---- the input contigs' set orders, through S1's own path and before the new arena makes the cached ones stale ----
    Carve C;
    const Seg s_mc = C.seg(sizeof(fl::MonoContig) * n), s_rp = C.seg(8ull * (n + 1)), s_so = C.seg(8ull * (n + 1)), s_ws = C.seg(32 * S + 32), s_zk = C.seg(4 * S + 4), s_rm = C.seg(S + 16),
              s_nr = C.seg(8ull * n), s_k3 = C.seg(12 * Rin + 16), s_cdev = C.seg(sizeof(fl::ContigDev) * n), s_uc = C.seg(sizeof(fl::UploadContig) * n), s_op = C.seg(8ull * (n + 1)),
              s_or = C.seg(4 * Rin + 16), s_st = C.seg(sizeof(fl::UploadStatus) * n), s_sop = C.seg(8ull * n), s_spp = C.seg(8ull * n);
    if (int rc = C.place(ctx->mono_buf)) return rc;
    int t = 0;
    if (with_set_order && Rin) {
        std::vector<fl::ContigDev> cdev(n); std::vector<uint64_t> ncells(n); uint32_t len_max = 1;
        for (uint32_t i = 0; i < n; ++i) { cdev[i] = contigs[i]->dev; ncells[i] = contigs[i]->n_cells; len_max = std::max(len_max, contigs[i]->max_len); }
        t = T.begin(K_H2D);
        HIPCHK(C.up(s_cdev, cdev.data(), sizeof(fl::ContigDev) * n, ctx->stream));
        T.end(t);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        t = T.begin(K_ORDER);
        const int orc = cell_orders(ctx, C.at<const fl::ContigDev>(s_cdev), cdev, ncells, len_max);
        T.end(t);
        if (orc) { sync_all(ctx); return orc; }
    }
    // ---- count, decide, COUNT: three words per input read come back ----
    std::vector<fl::MonoContig> mc(n);
    for (uint32_t i = 0; i < n; ++i) {
        const floria_hip_contig* k = contigs[i];
        fl::MonoContig& m = mc[i];
        m.read_off = k->dev.read_off; m.snp = k->dev.cell_snp; m.cell_aw = k->dev.cell_aw; m.snp_base = snp_off[i]; m.ord_base = cpi[i]; m.seq_pos = k->seq_pos;
        m.n_reads = k->n_reads; m.n_cells = (uint32_t)k->n_cells; m.n_snps = (uint32_t)std::min<uint64_t>(snp_off[i + 1] - snp_off[i], 0xffffffffull); m.pad = 0;
    }
    fl::MonoArgs a{};
    a.contigs = C.at<const fl::MonoContig>(s_mc); a.read_prefix = C.at<const uint64_t>(s_rp); a.snp_off = C.at<const uint64_t>(s_so); a.wsum = C.at<unsigned long long>(s_ws);
    a.zero_key = C.at<uint32_t>(s_zk); a.removed = C.at<uint8_t>(s_rm); a.n_removed = C.at<unsigned long long>(s_nr); a.keep3 = C.at<uint32_t>(s_k3);
    a.error = error; a.n_reads_in = Rin; a.n_snps_total = S; a.n_contigs = n;
    t = T.begin(K_H2D);
    HIPCHK(C.up(s_mc, mc.data(), sizeof(fl::MonoContig) * n, ctx->stream)); HIPCHK(C.up(s_rp, rp.data(), 8ull * (n + 1), ctx->stream)); HIPCHK(C.up(s_so, snp_off, 8ull * (n + 1), ctx->stream));
    T.end(t);
    t = T.begin(K_CLEAR);
    HIPCHK(hipMemsetAsync(C.at(s_ws), 0, s_ws.bytes, ctx->stream)); HIPCHK(hipMemsetAsync(C.at(s_zk), 0, s_zk.bytes, ctx->stream));
    HIPCHK(hipMemsetAsync(C.at(s_rm), 0, s_rm.bytes, ctx->stream)); HIPCHK(hipMemsetAsync(C.at(s_nr), 0, 8ull * n, ctx->stream));
    T.end(t);
    const unsigned wgs_in = (unsigned)((Rin + fl::UP_READS_PER_WG - 1) / fl::UP_READS_PER_WG);
    std::vector<uint32_t> k3(3 * Rin);
    std::vector<unsigned long long> n_rm(n, 0);
    if (Rin) {
        t = T.begin(K_COUNT); hipLaunchKernelGGL(fl::mono_count_kernel, dim3(wgs_in), dim3(64), 0, ctx->stream, a); T.end(t);
        HIPCHK(hipGetLastError());
        if (S) { t = T.begin(K_DECIDE); hipLaunchKernelGGL(fl::mono_decide_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, a); T.end(t); }
        HIPCHK(hipGetLastError());
        t = T.begin(K_FCOUNT); hipLaunchKernelGGL(fl::mono_filter_kernel<false>, dim3(wgs_in), dim3(64), 0, ctx->stream, a); T.end(t);
        HIPCHK(hipGetLastError());
        t = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(k3.data(), C.at(s_k3), 12 * Rin, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(n_rm.data(), C.at(s_nr), 8ull * n, hipMemcpyDeviceToHost, ctx->stream));
        T.end(t);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // ---- the host's part: drop the empty reads, Frag::cmp with the old index, prefix sums ----
    std::vector<uint64_t> rpo(n + 1, 0), cpo(n + 1, 0);       // output reads / cells before contig c
    std::vector<uint32_t> old_read; old_read.reserve(Rin);
    std::vector<uint32_t> ro_all;                              // the output contigs' read_off arrays as the arena holds them: contig c's [n_reads + 1] entries start at rp[c] + c
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t* k = k3.data() + 3 * rp[c];
        const size_t at = old_read.size();
        for (uint32_t r = 0; r < contigs[c]->n_reads; ++r) if (k[3 * (size_t)r]) old_read.push_back(r);
        std::stable_sort(old_read.begin() + at, old_read.end(), [&](uint32_t x, uint32_t y) {
            const uint32_t fx = k[3 * (size_t)x + 1], fy = k[3 * (size_t)y + 1], lx = k[3 * (size_t)x + 2], ly = k[3 * (size_t)y + 2];
            return fx != fy ? fx < fy : lx > ly;
        });
        uint64_t cells = 0;
        ro_all.push_back(0);
        for (size_t i = at; i < old_read.size(); ++i) { cells += k[3 * (size_t)old_read[i]]; ro_all.push_back((uint32_t)cells); }
        if (cells > contigs[c]->n_cells) return fail(FLORIA_E_DEVICE, "drop_monomorphic: a contig's surviving cells outnumber its cells");
        rpo[c + 1] = old_read.size(); cpo[c + 1] = cpo[c] + cells;
    }
    const uint64_t R = rpo[n], CC = cpo[n];
    // ---- the arena, as an upload of a CSR batch of these sizes would have it.  FILL writes the resident form, so no raw bytes exist and the tables stay in mono_buf ----
    const bool any_so = with_set_order != 0 && CC != 0;
    bool any_sp = false;                                       // an output contig carries positions iff its input does
    for (uint32_t i = 0; i < n; ++i) any_sp = any_sp || contigs[i]->seq_pos != nullptr;
    UploadPlan P;
    if (int rc = P.open(ctx, n, std::move(rpo), std::move(cpo), any_so, any_sp, out, false)) return rc;
    std::vector<uint32_t*> sop(n, nullptr), spp(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        if (contigs[i]->seq_pos) P.sp_dev[i] = spp[i] = P.sp_at(i);
        if (any_so && P.ucd[i].n_reads) P.so_dev[i] = sop[i] = P.so_at(i);
    }
    a.out = C.at<const fl::UploadContig>(s_uc); a.out_prefix = C.at<const uint64_t>(s_op); a.old_read = C.at<const uint32_t>(s_or); a.status = C.at<fl::UploadStatus>(s_st);
    a.Rq1 = ctx->d_hash.as<uint64_t>(); a.Rq2 = ctx->d_hash.as<uint64_t>() + 2ull * ctx->hash_len;
    a.out_set_order = C.at<uint32_t* const>(s_sop); a.ord = ctx->cur_ord; a.n_reads_out = R;
    a.out_seq_pos = any_sp ? C.at<uint32_t* const>(s_spp) : nullptr;
    t = T.begin(K_H2D);
    HIPCHK_AS("drop_monomorphic: ", C.up(s_uc, P.ucd.data(), sizeof(fl::UploadContig) * n, ctx->stream));
    HIPCHK_AS("drop_monomorphic: ", C.up(s_op, P.rp.data(), 8ull * (n + 1), ctx->stream));
    HIPCHK_AS("drop_monomorphic: ", C.up(s_or, old_read.data(), 4 * R, ctx->stream));
    HIPCHK_AS("drop_monomorphic: ", C.up(s_st, P.ust.data(), sizeof(fl::UploadStatus) * n, ctx->stream));
    HIPCHK_AS("drop_monomorphic: ", C.up(s_sop, sop.data(), 8ull * n, ctx->stream));
    if (any_sp) HIPCHK_AS("drop_monomorphic: ", C.up(s_spp, spp.data(), 8ull * n, ctx->stream));
    if (R) HIPCHK_AS("drop_monomorphic: ", hipMemcpyAsync(P.D + P.Y.o_ro, ro_all.data(), 4 * ro_all.size(), hipMemcpyHostToDevice, ctx->stream));
    T.end(t);
    if (R) {
        const uint32_t grid = items_grid(ctx, R, 4);      // one wavefront per output read
        t = T.begin(K_FILL);
        hipLaunchKernelGGL(fl::mono_filter_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
        T.end(t);
        if (any_so) { t = T.begin(K_ORDER); hipLaunchKernelGGL(fl::mono_order_kernel, dim3(grid), dim3(256), 0, ctx->stream, a); T.end(t); }
        HIPCHK_AS("drop_monomorphic: ", hipGetLastError());
    }
    t = T.begin(K_D2H);
    HIPCHK_AS("drop_monomorphic: ", hipMemcpyAsync(P.ust.data(), C.at(s_st), sizeof(fl::UploadStatus) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (res) {
        if (!new_result(R, S)) return fail(FLORIA_E_NOMEM, "calloc");
        if (S) HIPCHK_AS("drop_monomorphic: ", hipMemcpyAsync(M->removed, C.at(s_rm), S, hipMemcpyDeviceToHost, ctx->stream));
    }
    T.end(t);
    HIPCHK_AS("drop_monomorphic: ", hipStreamSynchronize(ctx->stream));
    if (M) {
        memcpy(M->read_off, P.rp.data(), 8ull * (n + 1));
        if (R) memcpy(M->old_read, old_read.data(), 4 * R);
        for (uint32_t c = 0; c < n; ++c) {                      // the survivors' new ends: the COUNT pass brought them back with the cell counts
            const uint32_t* k = k3.data() + 3 * rp[c];
            for (uint64_t i = P.rp[c]; i < P.rp[c + 1]; ++i) { M->new_first[i] = k[3 * (size_t)old_read[i] + 1]; M->new_last[i] = k[3 * (size_t)old_read[i] + 2]; }
        }
        for (uint32_t c = 0; c < n; ++c) M->n_removed_snps += n_rm[c];
        M->n_removed_cells = cpi[n] - CC; M->n_dropped_reads = Rin - R;
    }
    if (int rc = P.commit()) return rc;
    T.publish(ctx->timing);
    const int kinds[6] = {K_CLEAR, K_COUNT, K_DECIDE, K_FCOUNT, K_FILL, K_ORDER};
    for (int k = 0; k < 6; ++k) { ctx->mono_ms[k] = T.sum(kinds[k]); ctx->timing.pileup_ms += ctx->mono_ms[k]; }
    if (res) { *res = M; M = nullptr; }
    return 0;
}

// ---- allele tables of haplosets (stats_kernel.h: alleles_kernel) ------------------------------------------------------------------------------------------------
int floria_hip_haploset_alleles(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig, const uint64_t* grp_off,
                                const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups, const uint64_t* pos_off, uint32_t* counts) {
    if (!ctx || (n_contigs && !contigs) || (n_groups && (!grp_off || !grp_range || !pos_off))) return fail(FLORIA_E_INVALID, "null argument");
    if (n_groups == 0) return 0;
    if (grp_off[n_groups] && !grp_read) return fail(FLORIA_E_INVALID, "null argument");
    if (int rc = GroupTables::check(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, nullptr)) return rc;
    std::vector<fl::ContigDev> cdev(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) cdev[i] = contigs[i]->dev;
    GroupTables G{cdev.data(), sizeof(fl::ContigDev) * n_contigs, grp_contig, grp_off, grp_read, grp_range, n_groups};
    return alleles_core(ctx, grp_range, n_groups, pos_off, &G, DevGroups{}, counts);
}
}  // extern "C"

namespace {
int alleles_core(floria_hip_ctx* ctx, const uint32_t* grp_range, uint32_t n_groups, const uint64_t* pos_off, GroupTables* G, DevGroups dg, uint32_t* counts) {
    std::vector<uint64_t> hoff(n_groups + 1, 0);
    if (pos_off[0] != 0) return fail(FLORIA_E_INVALID, "haploset_alleles: pos_off does not start at 0");
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t lo = grp_range[2 * g], hi = grp_range[2 * g + 1];
        const uint64_t len = hi >= lo ? (uint64_t)(hi - lo) + 1 : 0;
        if (pos_off[g + 1] < pos_off[g] || pos_off[g + 1] - pos_off[g] != len)
            return fail(FLORIA_E_INVALID, "haploset_alleles: pos_off is not the prefix sum of the range lengths at group " + std::to_string(g));
        hoff[g + 1] = 4 * pos_off[g + 1];
    }
    const uint64_t n_counts = hoff[n_groups];
    if (n_counts == 0) return 0;
    if (!counts) return fail(FLORIA_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->batch_token = 0;                                  // misc is about to be overwritten (floria_hip_hap_graph checks the token)
    Carve C;
    if (G) G->carve(C, 4);
    const Seg s_ho = C.seg(8ull * (n_groups + 1)), s_h = C.seg(4ull * n_counts + 4);
    if (int rc = C.place(ctx->misc)) return rc;
    if (G) { if (int rc = G->up(C, ctx->stream)) return rc; dg = G->dev(C); }
    HIPCHK(C.up(s_ho, hoff.data(), 8ull * (n_groups + 1), ctx->stream));
    HIPCHK(hipMemsetAsync(C.at(s_h), 0, s_h.bytes, ctx->stream));
    fl::StatsArgs a{};
    a.contigs = (const fl::ContigDev*)dg.cd; a.grp_contig = dg.gc; a.grp_off = dg.go;
    a.grp_read = dg.gr; a.grp_range = dg.rg; a.hist_off = C.at<const uint64_t>(s_ho);
    a.hist = C.at<uint32_t>(s_h); a.out = nullptr; a.n_groups = n_groups;
    hipLaunchKernelGGL(fl::alleles_kernel, dim3(n_groups), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts, C.at(s_h), 4ull * n_counts, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace
extern "C" {

// ---- first / last sequence position of a read inside a haploset's SNP range (span_kernel.h) ----------------------------------------------------------------------
int floria_hip_read_spans(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig, const uint64_t* grp_off,
                          const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups, uint32_t* left, uint32_t* right) {
    if (!ctx || (n_contigs && !contigs) || (n_groups && (!grp_contig || !grp_off || !grp_range))) return fail(FLORIA_E_INVALID, "null argument");
    if (n_groups && grp_off[0] != 0) return fail(FLORIA_E_INVALID, "read_spans: grp_off does not start at 0");      // (here grp_read has grp_off[n_groups] entries: tested before any is read)
    if (int rc = GroupTables::check(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, "read_spans")) return rc;
    std::vector<fl::SpanContig> sc(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) {
        const floria_hip_contig* k = contigs[i];
        if (!k->seq_pos) return fail(FLORIA_E_INVALID, "the contig carries no seq_pos");
        sc[i] = fl::SpanContig{k->dev.read_off, k->dev.cell_snp, k->seq_pos, k->n_reads, (uint32_t)k->n_cells};
    }
    if (n_groups == 0) return 0;
    const uint64_t N = grp_off[n_groups];
    if (N == 0) return 0;
    if (!left || !right) return fail(FLORIA_E_INVALID, "null argument");
    GroupTables G{sc.data(), sizeof(fl::SpanContig) * n_contigs, grp_contig, grp_off, grp_read, grp_range, n_groups};
    return spans_core(ctx, n_contigs, N, n_groups, &G, DevGroups{}, left, right);
}
}  // extern "C"

namespace {
int spans_core(floria_hip_ctx* ctx, uint32_t n_contigs, uint64_t N, uint32_t n_groups, GroupTables* G, DevGroups dg, uint32_t* left, uint32_t* right) {
    if (N >= (1ull << 32) * 256) return fail(FLORIA_E_UNSUPPORTED, "read_spans: 2^40 and more entries in one call");
    HIPCHK(hipSetDevice(ctx->device));
    Carve C;
    if (G) G->carve(C, 0);
    const Seg s_l = C.seg(4 * N), s_r = C.seg(4 * N);
    if (int rc = C.place(ctx->span_buf)) return rc;
    EventTimer T(ctx->stream);
    ctx->timing = floria_timing{};
    int t = T.begin(K_H2D);
    if (G) { if (int rc = G->up(C, ctx->stream)) return rc; dg = G->dev(C); }
    T.end(t);
    fl::SpanArgs a{};
    a.contigs = (const fl::SpanContig*)dg.cd; a.grp_contig = dg.gc; a.grp_off = dg.go; a.grp_read = dg.gr;
    a.grp_range = dg.rg; a.left = C.at<uint32_t>(s_l); a.right = C.at<uint32_t>(s_r); a.n_entries = N; a.n_groups = n_groups; a.n_contigs = n_contigs;
    t = T.begin(K_PILEUP);
    hipLaunchKernelGGL(fl::read_spans_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    T.end(t);
    t = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(left, a.left, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(right, a.right, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
    T.end(t);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    T.publish(ctx->timing);
    return 0;
}
}  // namespace
extern "C" {

// ---- get_hapq (part_block_manip.rs:517-616) for the haplosets of many contigs (the reference calls it once per contig) ----------
int floria_hip_hapq_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig,
                          const uint64_t* grp_off, const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups,
                          const uint64_t* const* snp_to_genome_pos, const uint32_t* n_snps, uint64_t block_length,
                          uint8_t* hapq, double* rel_err, double* avg_err) {
    if (!ctx || (n_contigs && (!contigs || !avg_err)) || (n_groups && (!grp_off || !grp_range || !hapq || !rel_err))) return fail(FLORIA_E_INVALID, "null argument");
    if (block_length == 0) return fail(FLORIA_E_INVALID, "block_length must be positive");
    for (uint32_t c = 0; c < n_contigs; ++c) {
        if (!contigs[c] || contigs[c]->ctx != ctx) return fail(FLORIA_E_INVALID, "bad contig handle");
        avg_err[c] = std::numeric_limits<double>::quiet_NaN();                   // 0. / 0. for a contig without haplosets (:540)
        if (int rc0 = host_meta(contigs[c])) return rc0;
    }
    if (n_groups == 0) return 0;
    // (1) get_errors_cov_from_frags per haploset (:529-539)
    std::vector<double> st(4ull * n_groups);
    int rc = floria_hip_haploset_stats(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, grp_range, n_groups, st.data());
    if (rc) return rc;
    std::vector<uint32_t> gc(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; ++g) gc[g] = grp_contig ? grp_contig[g] : 0;
    // spans of the haplosets' reads (the consensus haplotype has a key wherever a read has a cell)
    std::vector<uint32_t> lo(n_groups, 0), len(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const floria_hip_contig* c = contigs[gc[g]];
        uint32_t r0 = 0xffffffffu, r1 = 0;
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
            const uint32_t r = grp_read[i];                                 // (validated by floria_hip_haploset_stats)
            r0 = std::min(r0, c->h_first[r]); r1 = std::max(r1, c->h_last[r]);
        }
        if (!(r0 > r1)) { lo[g] = r0; len[g] = r1 - r0 + 1; }
    }
    std::vector<fl::ContigDev> cdev(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) cdev[c] = contigs[c]->dev;
    GroupTables G{cdev.data(), sizeof(fl::ContigDev) * n_contigs, grp_contig, grp_off, grp_read, nullptr, n_groups};
    return hapq_core(ctx, contigs, n_contigs, gc, grp_off, grp_range, n_groups, st, lo, len, snp_to_genome_pos, n_snps, block_length, &G, DevGroups{}, hapq, rel_err, avg_err);
}
}  // extern "C"

namespace {
// get_hapq behind the statistics and the read spans (lo / len per group: len 0 = a group without reads): gc, grp_off and grp_range are host arrays
int hapq_core(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const std::vector<uint32_t>& gc, const uint64_t* grp_off, const uint32_t* grp_range,
              uint32_t n_groups, const std::vector<double>& st, const std::vector<uint32_t>& lo, const std::vector<uint32_t>& len, const uint64_t* const* snp_to_genome_pos,
              const uint32_t* n_snps, uint64_t block_length, GroupTables* G, DevGroups dg, uint8_t* hapq, double* rel_err, double* avg_err) {
    int rc = 0;
    std::vector<double> weight(n_contigs, 0.), error(n_contigs, 0.);
    for (uint32_t g = 0; g < n_groups; ++g) {                                    // (accumulated in group order inside each contig, as the reference does)
        weight[gc[g]] += st[4ull * g + 3]; error[gc[g]] += st[4ull * g + 2];
    }
    for (uint32_t c = 0; c < n_contigs; ++c) avg_err[c] = error[c] / weight[c];
    // base ranges (:584-600)
    uint32_t A = 2;
    for (uint32_t c = 0; c < n_contigs; ++c) A = std::max(A, contigs[c]->n_alleles);
    std::vector<uint64_t> coff(n_groups + 1, 0), base_range(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (len[g]) {
            const uint32_t x1 = grp_range[2 * g], x2 = grp_range[2 * g + 1];
            const uint64_t* pos = snp_to_genome_pos ? snp_to_genome_pos[gc[g]] : nullptr;
            const uint32_t ns = n_snps ? n_snps[gc[g]] : 0;
            if (!pos || x1 == 0 || x2 == 0 || x1 > ns || x2 > ns) return fail(FLORIA_E_INVALID, "haploset range outside snp_to_genome_pos");
            base_range[g] = pos[x2 - 1] - pos[x1 - 1];
        }
        coff[g + 1] = coff[g] + len[g];
    }
    // (2) find_overlapping_blocks (:453-513) inside each contig: rust-lapper's half-open overlap, overlap_percent (:13-24) > 0.05
    std::vector<std::vector<uint32_t>> by_contig(n_contigs);
    for (uint32_t g = 0; g < n_groups; ++g) by_contig[gc[g]].push_back(g);
    std::vector<uint32_t> pi, pj;
    std::vector<double> pol;
    std::vector<uint64_t> pair_off(n_groups + 1, 0);
    {
        std::vector<std::vector<uint32_t>> pj_of(n_groups);
        std::vector<std::vector<double>> ol_of(n_groups);
        for (uint32_t c = 0; c < n_contigs; ++c)
            for (uint32_t i : by_contig[c]) {
                const uint32_t x1 = grp_range[2 * i], x2 = grp_range[2 * i + 1];
                for (uint32_t j : by_contig[c]) {
                    if (j == i) continue;
                    const uint32_t y1 = grp_range[2 * j], y2 = grp_range[2 * j + 1];
                    if (!(y1 < x2 && y2 > x1)) continue;
                    const uint32_t a = x2 - y1 + 1, b = y2 - x1 + 1;
                    double ol = (double)std::min(a, b) / (double)(x2 - x1 + 1);
                    if (ol > 1.) ol = 1.;
                    if (!(ol > 0.05)) continue;
                    pj_of[i].push_back(j); ol_of[i].push_back(ol);
                }
            }
        for (uint32_t i = 0; i < n_groups; ++i) {
            for (size_t x = 0; x < pj_of[i].size(); ++x) { pi.push_back(i); pj.push_back(pj_of[i][x]); pol.push_back(ol_of[i][x]); }
            pair_off[i + 1] = pi.size();
        }
    }
    const uint32_t n_pairs = (uint32_t)pi.size();
    std::vector<uint32_t> sd(2ull * n_pairs + 2, 0);
    if (n_pairs) {
        HIPCHK(hipSetDevice(ctx->device));
        ctx->batch_token = 0;
        Carve C;
        if (G) G->carve(C, 4);
        const Seg s_lo = C.seg(4ull * n_groups), s_len = C.seg(4ull * n_groups), s_co = C.seg(8ull * (n_groups + 1)), s_h = C.seg(8ull * coff[n_groups] * A + 8),
                  s_c = C.seg(coff[n_groups] + 8), s_pi = C.seg(4ull * n_pairs), s_pj = C.seg(4ull * n_pairs), s_sd = C.seg(8ull * n_pairs);
        rc = C.place(ctx->misc); if (rc) return rc;
        if (G) { rc = G->up(C, ctx->stream); if (rc) return rc; dg = G->dev(C); }
        HIPCHK(C.up(s_lo, lo.data(), 4ull * n_groups, ctx->stream)); HIPCHK(C.up(s_len, len.data(), 4ull * n_groups, ctx->stream)); HIPCHK(C.up(s_co, coff.data(), 8ull * (n_groups + 1), ctx->stream));
        HIPCHK(C.up(s_pi, pi.data(), 4ull * n_pairs, ctx->stream)); HIPCHK(C.up(s_pj, pj.data(), 4ull * n_pairs, ctx->stream));
        HIPCHK(hipMemsetAsync(C.at(s_h), 0, s_h.bytes, ctx->stream));
        fl::ConsensusArgs ca{};
        ca.contigs = (const fl::ContigDev*)dg.cd; ca.grp_contig = dg.gc;
        ca.grp_off = dg.go; ca.grp_read = dg.gr;
        ca.span_lo = C.at<const uint32_t>(s_lo); ca.span_len = C.at<const uint32_t>(s_len); ca.cons_off = C.at<const uint64_t>(s_co);
        ca.hist = C.at<unsigned long long>(s_h); ca.cons = C.at<uint8_t>(s_c); ca.n_groups = n_groups;
        if (A == 2) hipLaunchKernelGGL(fl::consensus_kernel<2>, dim3(n_groups), dim3(256), 0, ctx->stream, ca);
        else hipLaunchKernelGGL(fl::consensus_kernel<4>, dim3(n_groups), dim3(256), 0, ctx->stream, ca);
        HIPCHK(hipGetLastError());
        fl::PairArgs pa{};
        pa.pair_i = C.at<const uint32_t>(s_pi); pa.pair_j = C.at<const uint32_t>(s_pj); pa.span_lo = ca.span_lo; pa.span_len = ca.span_len;
        pa.cons_off = ca.cons_off; pa.cons = ca.cons; pa.same_diff = C.at<uint32_t>(s_sd); pa.n_pairs = n_pairs;
        hipLaunchKernelGGL(fl::pair_kernel, dim3(n_pairs), dim3(64), 0, ctx->stream, pa);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sd.data(), C.at(s_sd), 8ull * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    // (3) the scalar tail (:543-615), same operation order as the reference
    for (uint32_t i = 0; i < n_groups; ++i) {
        double max_penalty = 0.;
        for (uint64_t x = pair_off[i]; x < pair_off[i + 1]; ++x) {
            const double same = (double)sd[2 * x], diff = (double)sd[2 * x + 1];
            const double dist = (same + diff) == 0. ? 1. : diff / (same + diff);
            if (pol[x] * (1. - dist) > max_penalty) max_penalty = pol[x] * (1. - dist);
        }
        const uint64_t n_i = grp_off[i + 1] - grp_off[i];
        const double t1 = 40. * (1. - max_penalty);                                   // constants::HAPQ_CONSTANT
        const double t2 = std::min(1., (double)n_i / 3.);
        const double t3 = std::max(0.0, std::log(((double)base_range[i] / (double)block_length) + 1.));
        const double prod = t1 * t2 * t3;
        uint64_t hq = prod > 0. ? (prod >= 18446744073709551615. ? ~0ull : (uint64_t)prod) : 0;      // `as usize`: saturating, NaN -> 0
        if (n_i == 1) hq = 0;
        hapq[i] = (uint8_t)std::min<uint64_t>(hq, 60);
        rel_err[i] = st[4ull * i + 1] / avg_err[gc[i]];
    }
    return 0;
}
}  // namespace
extern "C" {

int floria_hip_hapq(floria_hip_ctx* ctx, const floria_hip_contig* contig, const uint64_t* grp_off, const uint32_t* grp_read,
                    const uint32_t* grp_range, uint32_t n_groups, const uint64_t* snp_to_genome_pos, uint32_t n_snps,
                    uint64_t block_length, uint8_t* hapq, double* rel_err, double* avg_err) {
    if (!contig || !avg_err) return fail(FLORIA_E_INVALID, "null argument");
    const floria_hip_contig* one[1] = {contig};
    const uint64_t* pos[1] = {snp_to_genome_pos};
    return floria_hip_hapq_batch(ctx, one, 1, nullptr, grp_off, grp_read, grp_range, n_groups, pos, &n_snps, block_length, hapq, rel_err, avg_err);
}

// ---- S2 --------------------------------------------------------------------------------------------------------
// process_reads_for_final_parts for MANY contigs in one launch (one wavefront per contig): the reference calls it once
// per contig from its serial contig loop (floria.rs:229,359-366); the chain is sequential inside a contig and independent
// across contigs.
}  // extern "C"

// The output of one S2 call, resident (include/floria_hip.h): the group tables the consumer kernels read and their two contig tables, in a buffer of its own.
struct floria_hip_haplosets {
    floria_hip_ctx* ctx = nullptr;
    std::vector<const floria_hip_contig*> contigs;                 // the handles the call was given, in its order
    DevBuf buf;
    uint64_t n_groups = 0, n_reads = 0;                            // over all contigs
    std::vector<uint64_t> c_groups, c_reads;                       // per contig: the one copy the S2 call makes
    uint32_t A = 2;
    const fl::ContigDev* d_cd = nullptr;
    const fl::SpanContig* d_sc = nullptr;                          // null unless every contig carries positions
    const uint32_t* d_gc = nullptr; const uint64_t* d_go = nullptr; const uint32_t *d_gr = nullptr, *d_rg = nullptr;
    uint32_t *d_lo = nullptr, *d_len = nullptr;                    // get_hapq's read spans per group (hs_span_kernel), computed on first use
    // header-sized host mirrors (16 B per group, never a read id), fetched from the device on first use: what the consumers' host parts size their tables by
    bool have_hdr = false, have_span = false;
    std::vector<uint64_t> h_off; std::vector<uint32_t> h_range, h_gc, h_lo, h_len;
    ~floria_hip_haplosets() { buf.release(); }
};

namespace {

int hs_headers(const floria_hip_haplosets* chs);
int hs_spans(floria_hip_ctx* ctx, const floria_hip_haplosets* chs);
struct S2Plan;
int s2_resident_core(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, S2Plan& P, const std::vector<uint64_t>& gb,
                     const std::vector<uint32_t>& in_contig, const std::vector<uint32_t>& in_range, const uint32_t* read_order, const uint64_t* order_off, double epsilon,
                     floria_hip_haplosets** out);

// S2 up to the re-insertion kernels, shared by floria_hip_reassign_batch and floria_hip_reassign_batch_resident: validation, the host prologue (read -> candidate
// groups, the `multi` list, p0 / p1), the call's segments in the context's scratch, the uploads and the launch with its path choice.  `assign` stays on the device.
struct S2Plan {
    uint32_t A = 2;
    std::vector<std::vector<uint32_t>> cg;                         // groups of each contig, in input order (contig-local group id = rank among the contig's groups)
    std::vector<uint64_t> r2g_off_base, r2g_base, grp_base, assign_base, r2g_off_all, hist_off_all, multi_off_all;
    std::vector<uint32_t> r2g_all, gpos0_all, multi_all;
    std::vector<uint32_t> rid_lo, rid_hi;                          // per group, contig-major as gpos0_all: the id window [lo, hi) of its input list (haploset_kernel.h)
    std::vector<fl::ContigDev> cdev;
    uint64_t hist_cells = 0, n_assign = 0;
    uint64_t n_ro = 0, n_r2g = 0, n_mu = 0;                        // entries of r2g_off / r2g / multi the call's segments hold
    const floria_hip_haplosets* src = nullptr;                     // non-null: the input groups are this handle's, and the per-read tables are built on the device (dev_tables)
    Seg s_cd{}, s_rob{}, s_rb{}, s_gb{}, s_ab{}, s_ro{}, s_r2g{}, s_ho{}, s_p0{}, s_hist{}, s_as{}, s_q{}, s_ord{}, s_oo{}, s_mu{}, s_mo{}, s_ls{};

    int prologue(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig, const uint64_t* grp_off,
                 const uint32_t* grp_read, uint32_t n_groups, const uint32_t* read_order, const uint64_t* order_off) {
    if (int rc = GroupTables::check(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, nullptr)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->timing = floria_timing{};
    ctx->batch_token = 0;                      // misc is about to be overwritten
    for (uint32_t i = 0; i < n_contigs; ++i) {
        A = std::max(A, contigs[i]->n_alleles);
        if (int rc0 = host_meta(contigs[i])) return rc0;
    }
    cg.assign(n_contigs, {});
    for (uint32_t g = 0; g < n_groups; ++g) cg[grp_contig ? grp_contig[g] : 0].push_back(g);
    r2g_off_base.assign(n_contigs, 0); r2g_base.assign(n_contigs, 0); grp_base.assign(n_contigs, 0); assign_base.assign(n_contigs, 0);
    cdev.assign(n_contigs, fl::ContigDev{});
    for (uint32_t ci = 0; ci < n_contigs; ++ci) {
        const floria_hip_contig* c = contigs[ci];
        cdev[ci] = c->dev;
        const uint32_t N = c->n_reads;
        // read -> groups (part_block_manip.rs:185-193) by counting sort: groups are visited in ascending local id, so every read's candidate
        // list comes out ascending; groups are sets (a repeated id inside one group counts once)
        std::vector<uint32_t> p0(cg[ci].size(), UINT32_MAX), p1(cg[ci].size(), 0), w0(cg[ci].size(), UINT32_MAX), w1(cg[ci].size(), 0);
        std::vector<uint64_t> off(N + 1, 0);
        std::vector<uint32_t> last(N, UINT32_MAX);
        for (uint32_t lg = 0; lg < cg[ci].size(); ++lg) {
            const uint32_t g = cg[ci][lg];
            for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
                const uint32_t r = grp_read[i];                                 // (validated above)
                w0[lg] = std::min(w0[lg], r); w1[lg] = std::max(w1[lg], r + 1);
                if (last[r] == lg) continue;
                last[r] = lg;
                off[r + 1]++;
                p0[lg] = std::min(p0[lg], c->h_first[r]); p1[lg] = std::max(p1[lg], c->h_last[r]);
            }
        }
        for (uint32_t r = 0; r < N; ++r) off[r + 1] += off[r];
        r2g_off_base[ci] = r2g_off_all.size(); r2g_base[ci] = r2g_all.size(); grp_base[ci] = gpos0_all.size(); assign_base[ci] = n_assign;
        {
            const size_t base = r2g_all.size();
            r2g_all.resize(base + off[N]);
            std::vector<uint64_t> fill(off.begin(), off.end() - 1);
            std::fill(last.begin(), last.end(), UINT32_MAX);
            for (uint32_t lg = 0; lg < cg[ci].size(); ++lg) {
                const uint32_t g = cg[ci][lg];
                for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
                    const uint32_t r = grp_read[i];
                    if (last[r] == lg) continue;
                    last[r] = lg;
                    r2g_all[base + fill[r]++] = lg;
                }
            }
        }
        if (read_order) {                                   // every read that sits in a group must be visited exactly once
            std::vector<uint8_t> seen(N, 0);
            for (uint64_t i = order_off[ci]; i < order_off[ci + 1]; ++i) {
                const uint32_t r = read_order[i];
                if (r >= N || seen[r]) return fail(FLORIA_E_INVALID, "read_order: id out of range or repeated");
                seen[r] = 1;
            }
            for (uint32_t r = 0; r < N; ++r) if (off[r + 1] > off[r] && !seen[r]) return fail(FLORIA_E_INVALID, "read_order misses a read that sits in a group");
        }
        multi_off_all.push_back(multi_all.size());
        {                                                   // visiting indices of the reads that have a choice (more than one candidate group)
            const uint64_t nv = read_order ? order_off[ci + 1] - order_off[ci] : N;
            for (uint64_t v = 0; v < nv; ++v) { const uint32_t r = read_order ? read_order[order_off[ci] + v] : (uint32_t)v; if (off[r + 1] - off[r] > 1) multi_all.push_back((uint32_t)v); }
        }
        r2g_off_all.insert(r2g_off_all.end(), off.begin(), off.end());
        for (uint32_t lg = 0; lg < cg[ci].size(); ++lg) {
            hist_off_all.push_back(hist_cells);
            gpos0_all.push_back(p0[lg] == UINT32_MAX ? 0 : p0[lg]);
            rid_lo.push_back(w0[lg] == UINT32_MAX ? 0 : w0[lg]); rid_hi.push_back(w1[lg]);
            hist_cells += p0[lg] == UINT32_MAX ? 0 : (uint64_t)(p1[lg] - p0[lg] + 1) * A;
        }
        n_assign += N;
    }
    multi_off_all.push_back(multi_all.size());
    n_ro = r2g_off_all.size(); n_r2g = r2g_all.size(); n_mu = multi_all.size();
    return 0;
    }

    // The second way to fill the tables: the input groups are a handle's (floria_hip_reassign_haplosets_resident).  The host part reads header-sized data only — per
    // group its size and the SNP span of its reads (the handle's mirrors: hs_headers, hs_spans) — and sizes the segments; the per-read tables (read -> groups, `multi`)
    // are built on the device inside run() (dev_tables).  Reads are visited in ascending id.  No first / last comes to the host (no host_meta).
    int prologue_handle(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* in) {
        HIPCHK(hipSetDevice(ctx->device));
        ctx->timing = floria_timing{};
        if (int rc = hs_headers(in)) return rc;
        if (int rc = hs_spans(ctx, in)) return rc;
        ctx->batch_token = 0;                      // misc is about to be overwritten
        src = in;
        r2g_off_base.assign(n_contigs, 0); r2g_base.assign(n_contigs, 0); grp_base.assign(n_contigs, 0); assign_base.assign(n_contigs, 0);
        cdev.assign(n_contigs, fl::ContigDev{});
        for (uint32_t i = 0; i < n_contigs; ++i) A = std::max(A, contigs[i]->n_alleles);
        uint64_t g = 0;
        for (uint32_t ci = 0; ci < n_contigs; ++ci) {
            cdev[ci] = contigs[ci]->dev;
            grp_base[ci] = g; assign_base[ci] = n_assign; r2g_off_base[ci] = n_assign + ci;      // (haploset_kernel.h: n_reads + 1 slots per contig, r2g_base stays 0)
            for (uint64_t k = 0; k < in->c_groups[ci]; ++k, ++g) {
                hist_off_all.push_back(hist_cells);
                gpos0_all.push_back(in->h_lo[g]);
                hist_cells += (uint64_t)in->h_len[g] * A;
            }
            n_assign += contigs[ci]->n_reads;
        }
        n_ro = n_assign + n_contigs; n_r2g = in->n_reads; n_mu = in->n_reads / 2;      // (a read with a choice sits in two groups at the least)
        if (n_ro >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "reassign_haplosets_resident: 2^32 and more reads in one call");
        return 0;
    }

    // ... and its device part, into the segments run() would upload: read -> groups offsets and lists, `multi` and its offsets (haploset_kernel.h).  The per-contig
    // `multi` counts come back for the path choice: one word per contig.
    int dev_tables(floria_hip_ctx* ctx, uint32_t n_contigs, const Carve& C, EventTimer& T) {
        const uint32_t n_groups = (uint32_t)src->n_groups;
        Carve S;
        const uint32_t tiles = (uint32_t)((n_ro + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE);
        const Seg s_mf = S.seg(8ull * n_ro + 8), s_ti = S.seg(8ull * tiles + 8);
        if (int rc = S.place(ctx->hs_tmp)) return rc;
        fl::HpArgs a{};
        a.contigs = C.at<const fl::ContigDev>(s_cd); a.grp_contig = src->d_gc; a.grp_off = src->d_go; a.grp_read = src->d_gr;
        a.grp_base = C.at<const uint64_t>(s_gb); a.ro_base = C.at<const uint64_t>(s_rob); a.ro = C.at<uint64_t>(s_ro); a.mf = S.at<uint64_t>(s_mf);
        a.cursor = C.at<uint32_t>(s_as); a.r2g = C.at<uint32_t>(s_r2g); a.multi = C.at<uint32_t>(s_mu); a.multi_off = C.at<uint64_t>(s_mo);
        a.n_slots = n_ro; a.n_entries = n_r2g; a.n_multi_cap = n_mu; a.n_groups = n_groups; a.n_contigs = n_contigs;
        HIPCHK(hipMemsetAsync(a.ro, 0, 8ull * n_ro + 8, ctx->stream));
        HIPCHK(hipMemsetAsync(a.cursor, 0, 4ull * n_assign + 4, ctx->stream));
        const uint32_t grid_g = items_grid(ctx, n_groups, 4), grid_s = items_grid(ctx, n_ro, 256);
        int tk = T.begin(K_SEL);
        hipLaunchKernelGGL(fl::hp_groups_kernel<false>, dim3(grid_g), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(fl::hp_flag_kernel, dim3(grid_s), dim3(256), 0, ctx->stream, a);
        launch_offset_scan(ctx, a.ro, S.at<uint64_t>(s_ti), (uint32_t)n_ro);
        launch_offset_scan(ctx, a.mf, S.at<uint64_t>(s_ti), (uint32_t)n_ro);
        hipLaunchKernelGGL(fl::hp_groups_kernel<true>, dim3(grid_g), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(fl::hp_sort_kernel, dim3(grid_s), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(fl::hp_multi_off_kernel, dim3(items_grid(ctx, n_contigs + 1, 256)), dim3(256), 0, ctx->stream, a);
        T.end(tk);
        HIPCHK(hipGetLastError());
        multi_off_all.assign(n_contigs + 1, 0);
        int td = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(multi_off_all.data(), a.multi_off, 8ull * (n_contigs + 1), hipMemcpyDeviceToHost, ctx->stream));
        T.end(td);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (multi_off_all.back() > n_mu) return fail(FLORIA_E_DEVICE, "reassign_haplosets_resident: the device's read tables are inconsistent");
        return 0;
    }

    // the call's segments, first in the caller's Carve (it may add its own behind them before it places the Carve in ctx->misc)
    void carve(Carve& C, uint32_t n_contigs, const uint32_t* read_order, const uint64_t* order_off) {
        s_cd = C.seg(sizeof(fl::ContigDev) * n_contigs); s_rob = C.seg(8ull * n_contigs); s_rb = C.seg(8ull * n_contigs); s_gb = C.seg(8ull * n_contigs);
        s_ab = C.seg(8ull * n_contigs); s_ro = C.seg(8ull * n_ro + 8); s_r2g = C.seg(4ull * n_r2g + 4);
        s_ho = C.seg(8ull * hist_off_all.size() + 8); s_p0 = C.seg(4ull * gpos0_all.size() + 4); s_hist = C.seg(8ull * hist_cells + 8);
        s_as = C.seg(4ull * n_assign + 4); s_q = C.seg(16); s_ord = C.seg(read_order ? 4ull * order_off[n_contigs] + 4 : 4);
        s_oo = C.seg(8ull * (n_contigs + 1)); s_mu = C.seg(4ull * n_mu + 4); s_mo = C.seg(8ull * (n_contigs + 1)); s_ls = C.seg(4ull * n_contigs + 4);
    }

    // uploads + the re-insertion launches, timed into T (K_H2D, K_REASSIGN); the caller goes on in the same stream
    int run(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const Carve& C, EventTimer& T, const uint32_t* read_order,
            const uint64_t* order_off, double epsilon) {
        int rc = 0;
        int th = T.begin(K_H2D);
        HIPCHK(C.up(s_cd, cdev.data(), sizeof(fl::ContigDev) * n_contigs, ctx->stream));
        HIPCHK(C.up(s_rob, r2g_off_base.data(), 8ull * n_contigs, ctx->stream)); HIPCHK(C.up(s_rb, r2g_base.data(), 8ull * n_contigs, ctx->stream));
        HIPCHK(C.up(s_gb, grp_base.data(), 8ull * n_contigs, ctx->stream)); HIPCHK(C.up(s_ab, assign_base.data(), 8ull * n_contigs, ctx->stream));
        if (!src) { HIPCHK(C.up(s_ro, r2g_off_all.data(), 8ull * r2g_off_all.size(), ctx->stream)); HIPCHK(C.up(s_r2g, r2g_all.data(), 4ull * r2g_all.size(), ctx->stream)); }
        HIPCHK(C.up(s_ho, hist_off_all.data(), 8ull * hist_off_all.size(), ctx->stream)); HIPCHK(C.up(s_p0, gpos0_all.data(), 4ull * gpos0_all.size(), ctx->stream));
        if (src) { T.end(th); rc = dev_tables(ctx, n_contigs, C, T); if (rc) return rc; th = T.begin(K_H2D); }      // (its cursors lie in `assign`: before the memset below)
        HIPCHK(hipMemsetAsync(C.at(s_hist), 0, s_hist.bytes, ctx->stream));
        HIPCHK(hipMemsetAsync(C.at(s_q), 0, 16, ctx->stream));
        HIPCHK(hipMemsetAsync(C.at(s_as), 0xff, s_as.bytes, ctx->stream));            // -1 = not assigned
        if (read_order) { HIPCHK(C.up(s_ord, read_order, 4ull * order_off[n_contigs], ctx->stream)); HIPCHK(C.up(s_oo, order_off, 8ull * (n_contigs + 1), ctx->stream)); }
        if (!src) { HIPCHK(C.up(s_mu, multi_all.data(), 4ull * multi_all.size(), ctx->stream)); HIPCHK(C.up(s_mo, multi_off_all.data(), 8ull * (n_contigs + 1), ctx->stream)); }
        T.end(th);
        fl::ReassignArgs a{};
        a.contigs = C.at<const fl::ContigDev>(s_cd); a.n_contigs = n_contigs;
        a.r2g_off_base = C.at<const uint64_t>(s_rob); a.r2g_off = C.at<const uint64_t>(s_ro);
        a.r2g_base = C.at<const uint64_t>(s_rb); a.r2g = C.at<const uint32_t>(s_r2g);
        a.grp_base = C.at<const uint64_t>(s_gb); a.grp_hist_off = C.at<const uint64_t>(s_ho); a.grp_pos0 = C.at<const uint32_t>(s_p0);
        a.hist = C.at<uint64_t>(s_hist); a.assign = C.at<int32_t>(s_as); a.assign_base = C.at<const uint64_t>(s_ab);
        a.eps = epsilon; a.queue_head = C.at<uint32_t>(s_q);
        a.order = read_order ? C.at<const uint32_t>(s_ord) : nullptr; a.order_off = C.at<const uint64_t>(s_oo);
        a.multi = C.at<const uint32_t>(s_mu); a.multi_off = C.at<const uint64_t>(s_mo);
        const bool arith = ctx->knobs.arith != 0;
        if (arith) {                                // the reference's running sums: every read's cells in the order of its position set
            std::vector<uint64_t> ncells(n_contigs); uint32_t len_max = 1;
            for (uint32_t ci = 0; ci < n_contigs; ++ci) { ncells[ci] = contigs[ci]->n_cells; len_max = std::max(len_max, contigs[ci]->max_len); }
            rc = cell_orders(ctx, a.contigs, cdev, ncells, len_max); if (rc) return rc;
            a.cell_ord = ctx->cur_ord; a.cell_ord_off = ctx->cur_ord_off;
        }
        // contigs where at least 1 read in 8 has a choice take the latency-optimised chain kernel, the others the parallel one
        std::vector<uint32_t> list_par, list_chain;
        for (uint32_t ci = 0; ci < n_contigs; ++ci) {
            const uint64_t nm = multi_off_all[ci + 1] - multi_off_all[ci];
            const uint64_t nv = read_order ? order_off[ci + 1] - order_off[ci] : contigs[ci]->n_reads;
            const bool chain = !arith && (ctx->knobs.reassign_path == 2 || (ctx->knobs.reassign_path == 0 && nm * 8 >= nv && nm > 0));
            (chain ? list_chain : list_par).push_back(ci);
        }
        std::vector<uint32_t> lists(list_par);
        lists.insert(lists.end(), list_chain.begin(), list_chain.end());
        HIPCHK(C.up(s_ls, lists.data(), 4ull * lists.size(), ctx->stream));
        int tk = T.begin(K_REASSIGN);
        if (!list_par.empty()) {
            a.list = C.at<const uint32_t>(s_ls); a.n_list = (uint32_t)list_par.size(); a.queue_head = C.at<uint32_t>(s_q);
            const uint32_t grid = std::min<uint32_t>(a.n_list, (uint32_t)ctx->n_cu * 8);
            if (arith) { if (A == 2) hipLaunchKernelGGL((fl::reassign_kernel<2, true>), dim3(grid), dim3(fl::REASSIGN_THREADS), 0, ctx->stream, a);
                         else hipLaunchKernelGGL((fl::reassign_kernel<4, true>), dim3(grid), dim3(fl::REASSIGN_THREADS), 0, ctx->stream, a); }
            else if (A == 2) hipLaunchKernelGGL(fl::reassign_kernel<2>, dim3(grid), dim3(fl::REASSIGN_THREADS), 0, ctx->stream, a);
            else hipLaunchKernelGGL(fl::reassign_kernel<4>, dim3(grid), dim3(fl::REASSIGN_THREADS), 0, ctx->stream, a);
        }
        if (!list_chain.empty()) {
            a.list = C.at<const uint32_t>(s_ls) + list_par.size(); a.n_list = (uint32_t)list_chain.size(); a.queue_head = C.at<uint32_t>(s_q) + 1;
            const uint32_t grid = std::min<uint32_t>(a.n_list, (uint32_t)ctx->n_cu * 16);
            if (A == 2) hipLaunchKernelGGL(fl::reassign_chain_kernel<2>, dim3(grid), dim3(64), 0, ctx->stream, a);
            else hipLaunchKernelGGL(fl::reassign_chain_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
        }
        ctx->timing.jobs = multi_off_all.back();                      // reads that had a choice (the sequential part of S2)
        T.end(tk);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

}  // namespace

extern "C" {

int floria_hip_reassign_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                              const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                              const uint32_t* grp_range, uint32_t n_groups, const uint32_t* read_order, const uint64_t* order_off,
                              double epsilon, floria_groups*** out) {
    if (!ctx || !out || (n_contigs && !contigs) || (n_groups && (!grp_off || !grp_range))) return fail(FLORIA_E_INVALID, "null argument");
    if ((read_order == nullptr) != (order_off == nullptr)) return fail(FLORIA_E_INVALID, "read_order and order_off go together");
    *out = nullptr;
    S2Plan P;
    if (int rc = P.prologue(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, read_order, order_off)) return rc;
    const std::vector<std::vector<uint32_t>>& cg = P.cg;
    const std::vector<uint64_t>& assign_base = P.assign_base;
    std::vector<int32_t> assign(P.n_assign, -1);
    if (P.n_assign && n_groups) {
        Carve C;
        P.carve(C, n_contigs, read_order, order_off);
        int rc = C.place(ctx->misc); if (rc) return rc;
        EventTimer T(ctx->stream);
        rc = P.run(ctx, contigs, n_contigs, C, T, read_order, order_off, epsilon); if (rc) return rc;
        int td = T.begin(K_D2H);
        HIPCHK(hipMemcpyAsync(assign.data(), C.at(P.s_as), 4ull * P.n_assign, hipMemcpyDeviceToHost, ctx->stream));
        T.end(td);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        T.publish(ctx->timing);
    }
    // ---- host bookkeeping per contig: rebuild groups, separate_broken_haplogroups (:27-98), sort_parts (:276-288) ----
    floria_groups** arr = (floria_groups**)calloc(std::max(1u, n_contigs), sizeof(floria_groups*));
    if (!arr) return fail(FLORIA_E_NOMEM, "calloc");
    for (uint32_t ci = 0; ci < n_contigs; ++ci) {
        const floria_hip_contig* c = contigs[ci];
        const uint32_t N = c->n_reads, ng = (uint32_t)cg[ci].size();
        std::vector<std::vector<uint32_t>> parts(ng);
        std::vector<std::pair<uint32_t, uint32_t>> ranges(ng);
        for (uint32_t lg = 0; lg < ng; ++lg) ranges[lg] = {grp_range[2 * cg[ci][lg]], grp_range[2 * cg[ci][lg] + 1]};
        const int32_t* as = assign.data() + assign_base[ci];
        for (uint32_t r = 0; r < N; ++r) if (as[r] >= 0) parts[as[r]].push_back(r);       // ascending id
        // Which read a split drops depends on the iteration order of the reference's FxHashSet among reads that share a first_position (:34-35, :62-63; measured:
        // every short-read contig of scripts/a14_sensitivity.py changes with it, no long-read one).  Here: ascending counter_id.  A host that wants its own sets'
        // order sets "s2_assign_only": it gets the haplogroups as re-inserted and runs these two cheap integer steps on its own sets.
        if (!ctx->knobs.s2_assign_only) {
            const auto& F = c->h_first; const auto& L = c->h_last;
            std::vector<std::pair<size_t, std::vector<uint32_t>>> all_breaks;
            const size_t n0 = ranges.size();
            for (size_t i = 0; i < n0; ++i) {
                uint32_t latest = 0;
                std::vector<uint32_t> breaks;
                for (uint32_t r : parts[i]) {                                // sorted by first_position (ids ascend)
                    if (latest != 0 && F[r] > latest && latest >= ranges[i].first && latest < ranges[i].second) breaks.push_back(latest);
                    if (L[r] > latest) latest = L[r];
                }
                if (!breaks.empty()) all_breaks.push_back({i, std::move(breaks)});
            }
            std::vector<std::vector<uint32_t>> new_parts;
            std::vector<std::pair<uint32_t, uint32_t>> new_ranges;
            for (auto& bi : all_breaks) {
                size_t spot = 0;
                uint32_t break_start = ranges[bi.first].first, end_spot = bi.second[0];
                std::vector<uint32_t> np;
                for (uint32_t r : parts[bi.first]) {
                    if (L[r] <= end_spot) np.push_back(r);
                    else {                                                   // :69-84: this read is not re-inserted
                        new_parts.push_back(std::move(np)); np.clear();
                        new_ranges.push_back({break_start, end_spot});
                        break_start = end_spot + 1;
                        ++spot;
                        end_spot = spot != bi.second.size() ? bi.second[spot] : UINT32_MAX;
                    }
                }
                new_parts.push_back(std::move(np));
                new_ranges.push_back({break_start, ranges[bi.first].second});
            }
            for (auto& bi : all_breaks) parts[bi.first].clear();
            for (size_t i = 0; i < new_parts.size(); ++i) { parts.push_back(std::move(new_parts[i])); ranges.push_back(new_ranges[i]); }
        }
        std::vector<size_t> idx(parts.size());
        std::iota(idx.begin(), idx.end(), 0);
        if (!ctx->knobs.s2_assign_only) std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return ranges[x] < ranges[y]; });
        floria_groups* G = (floria_groups*)calloc(1, sizeof(floria_groups));
        if (!G) { floria_hip_groups_array_free(arr, n_contigs); return fail(FLORIA_E_NOMEM, "calloc"); }
        arr[ci] = G;
        G->n_groups = (uint32_t)parts.size();
        G->grp_off = (uint64_t*)calloc(parts.size() + 1, 8);
        G->range = (uint32_t*)calloc(2 * parts.size() + 2, 4);
        uint64_t tot = 0;
        for (size_t k = 0; k < idx.size(); ++k) { G->grp_off[k] = tot; tot += parts[idx[k]].size(); G->range[2 * k] = ranges[idx[k]].first; G->range[2 * k + 1] = ranges[idx[k]].second; }
        G->grp_off[idx.size()] = tot;
        G->grp_read = (uint32_t*)malloc(4 * (tot + 1));
        for (size_t k = 0; k < idx.size(); ++k) std::copy(parts[idx[k]].begin(), parts[idx[k]].end(), G->grp_read + G->grp_off[k]);
    }
    *out = arr;
    return 0;
}

int floria_hip_reassign_ordered(floria_hip_ctx* ctx, const floria_hip_contig* c, const uint64_t* grp_off, const uint32_t* grp_read,
                                const uint32_t* grp_range, uint32_t n_groups, const uint32_t* read_order, uint32_t n_order,
                                double epsilon, floria_groups** out) {
    if (!c || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    const floria_hip_contig* arr[1] = {c};
    const uint64_t oo[2] = {0, n_order};
    floria_groups** res = nullptr;
    int rc = floria_hip_reassign_batch(ctx, arr, 1, nullptr, grp_off, grp_read, grp_range, n_groups, read_order, read_order ? oo : nullptr, epsilon, &res);
    if (rc) return rc;
    *out = res[0];
    free(res);
    return 0;
}
int floria_hip_reassign(floria_hip_ctx* ctx, const floria_hip_contig* c, const uint64_t* grp_off, const uint32_t* grp_read,
                        const uint32_t* grp_range, uint32_t n_groups, double epsilon, floria_groups** out) {
    return floria_hip_reassign_ordered(ctx, c, grp_off, grp_read, grp_range, n_groups, nullptr, 0, epsilon, out);
}
void floria_hip_groups_array_free(floria_groups** arr, uint32_t n) {
    if (!arr) return;
    for (uint32_t i = 0; i < n; ++i) floria_hip_groups_free(arr[i]);
    free(arr);
}
void floria_hip_groups_free(floria_groups* g) { if (g) { free(g->grp_off); free(g->grp_read); free(g->range); free(g); } }

}  // extern "C"

// ---- S2 with its epilogue on the device, and the haplosets as a handle (haploset_kernel.h) ---------------------------------------------------------------------
namespace {

// a handle's header mirror: grp_off and range per group from the device (16 B per group), grp_contig from the per-contig counts
int hs_headers(const floria_hip_haplosets* chs) {
    floria_hip_haplosets* hs = const_cast<floria_hip_haplosets*>(chs);
    if (hs->have_hdr) return 0;
    const uint64_t n = hs->n_groups;
    hs->h_off.assign(n + 1, 0); hs->h_range.assign(2 * n, 0); hs->h_gc.assign(n, 0);
    uint64_t g = 0;
    for (uint32_t c = 0; c < hs->c_groups.size(); ++c) for (uint64_t i = 0; i < hs->c_groups[c]; ++i) hs->h_gc[g++] = c;
    if (n) {
        HIPCHK(hipSetDevice(hs->ctx->device));
        HIPCHK(hipMemcpyAsync(hs->h_off.data(), hs->d_go, 8 * (n + 1), hipMemcpyDeviceToHost, hs->ctx->stream));
        HIPCHK(hipMemcpyAsync(hs->h_range.data(), hs->d_rg, 8 * n, hipMemcpyDeviceToHost, hs->ctx->stream));
        HIPCHK(hipStreamSynchronize(hs->ctx->stream));
    }
    hs->have_hdr = true;
    return 0;
}

// min first / max last of every haploset's reads (get_hapq; the histogram windows of an S2 call that takes the handle as its input), once per handle: 8 B per group come back
int hs_spans(floria_hip_ctx* ctx, const floria_hip_haplosets* chs) {
    floria_hip_haplosets* hs = const_cast<floria_hip_haplosets*>(chs);
    if (hs->have_span) return 0;
    const uint32_t n_groups = (uint32_t)hs->n_groups;
    hs->h_lo.assign(n_groups, 0); hs->h_len.assign(n_groups, 0);
    if (n_groups) {
        HIPCHK(hipSetDevice(ctx->device));
        hipLaunchKernelGGL(fl::hs_span_kernel, dim3(items_grid(ctx, n_groups, 4)), dim3(256), 0, ctx->stream, hs->d_cd, (uint32_t)hs->contigs.size(), hs->d_gc, hs->d_go, hs->d_gr, n_groups, hs->d_lo, hs->d_len);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs->h_lo.data(), hs->d_lo, 4ull * n_groups, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(hs->h_len.data(), hs->d_len, 4ull * n_groups, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    hs->have_span = true;
    return 0;
}

// what every call that takes a handle refuses before anything else
int hs_check(const floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs, const char* who) {
    if (!ctx || !hs || (n_contigs && !contigs)) return fail(FLORIA_E_INVALID, "null argument");
    if (hs->ctx != ctx) return fail(FLORIA_E_INVALID, std::string(who) + ": the haplosets belong to another context");
    if (n_contigs != hs->contigs.size()) return fail(FLORIA_E_INVALID, std::string(who) + ": " + std::to_string(n_contigs) + " contigs given, the haplosets were made from " + std::to_string(hs->contigs.size()));
    for (uint32_t i = 0; i < n_contigs; ++i) {
        if (!contigs[i]) return fail(FLORIA_E_INVALID, "null argument");
        if (contigs[i] != hs->contigs[i]) return fail(FLORIA_E_INVALID, std::string(who) + ": contig " + std::to_string(i) + " is not the one the haplosets were made from");
    }
    return 0;
}

DevGroups hs_dev(const floria_hip_haplosets* hs, bool span) { return DevGroups{span ? (const void*)hs->d_sc : (const void*)hs->d_cd, hs->d_gc, hs->d_go, hs->d_gr, hs->d_rg}; }

// a handle's buffer for NG groups and NR reads: carved, placed, its pointers set and its span table uploaded (`sc` must live until the stream has run); the contig
// table (cd) and the group arrays are the caller's to fill
struct HsSegs { Seg cd{}, sc{}, gc{}, go{}, gr{}, rg{}, lo{}, len{}; };
int hs_place(floria_hip_haplosets* hs, const floria_hip_contig* const* contigs, uint32_t n_contigs, uint64_t NG, uint64_t NR, Carve& H, HsSegs& S, std::vector<fl::SpanContig>& sc) {
    bool all_pos = true;
    sc.resize(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) {
        const floria_hip_contig* k = contigs[i];
        if (!k->seq_pos) all_pos = false;
        sc[i] = fl::SpanContig{k->dev.read_off, k->dev.cell_snp, k->seq_pos, k->n_reads, (uint32_t)k->n_cells};
    }
    S.cd = H.seg(sizeof(fl::ContigDev) * n_contigs); S.sc = H.seg(sizeof(fl::SpanContig) * n_contigs); S.gc = H.seg(4 * NG); S.go = H.seg(8 * (NG + 1));
    S.gr = H.seg(4 * NR + 4); S.rg = H.seg(8 * NG); S.lo = H.seg(4 * NG); S.len = H.seg(4 * NG);
    if (int rc = H.place(hs->buf)) return rc;
    if (all_pos) HIPCHK(H.up(S.sc, sc.data(), sizeof(fl::SpanContig) * n_contigs, hs->ctx->stream));
    hs->d_cd = H.at<const fl::ContigDev>(S.cd); hs->d_sc = all_pos ? H.at<const fl::SpanContig>(S.sc) : nullptr;
    hs->d_gc = H.at<const uint32_t>(S.gc); hs->d_go = H.at<const uint64_t>(S.go); hs->d_gr = H.at<const uint32_t>(S.gr); hs->d_rg = H.at<const uint32_t>(S.rg);
    hs->d_lo = H.at<uint32_t>(S.lo); hs->d_len = H.at<uint32_t>(S.len);
    return 0;
}

}  // namespace

extern "C" {

int floria_hip_reassign_batch_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                       const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                                       const uint32_t* grp_range, uint32_t n_groups, const uint32_t* read_order, const uint64_t* order_off,
                                       double epsilon, floria_hip_haplosets** out) {
    if (!ctx || !out || (n_contigs && !contigs) || (n_groups && (!grp_off || !grp_range))) return fail(FLORIA_E_INVALID, "null argument");
    if ((read_order == nullptr) != (order_off == nullptr)) return fail(FLORIA_E_INVALID, "read_order and order_off go together");
    *out = nullptr;
    S2Plan P;
    if (int rc = P.prologue(ctx, contigs, n_contigs, grp_contig, grp_off, grp_read, n_groups, read_order, order_off)) return rc;
    // the input groups contig-major, as the prologue numbers them
    const uint32_t n_in = n_groups;
    std::vector<uint64_t> gb(n_contigs + 1, 0);
    std::vector<uint32_t> in_contig(n_in), in_range(2ull * n_in);
    for (uint32_t ci = 0; ci < n_contigs; ++ci) {
        gb[ci + 1] = gb[ci] + P.cg[ci].size();
        for (uint32_t lg = 0; lg < P.cg[ci].size(); ++lg) {
            const uint64_t k = gb[ci] + lg; const uint32_t g = P.cg[ci][lg];
            in_contig[k] = ci; in_range[2 * k] = grp_range[2 * g]; in_range[2 * k + 1] = grp_range[2 * g + 1];
        }
    }
    return s2_resident_core(ctx, contigs, n_contigs, P, gb, in_contig, in_range, read_order, order_off, epsilon, out);
}

int floria_hip_reassign_haplosets_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* in, double epsilon,
                                           floria_hip_haplosets** out) {
    if (!out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (int rc = hs_check(ctx, contigs, n_contigs, in, "reassign_haplosets_resident")) return rc;
    if (in->n_groups >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "reassign_haplosets_resident: 2^32 and more haplosets in one call");
    S2Plan P;
    if (int rc = P.prologue_handle(ctx, contigs, n_contigs, in)) return rc;
    std::vector<uint64_t> gb(n_contigs + 1, 0);
    for (uint32_t ci = 0; ci < n_contigs; ++ci) gb[ci + 1] = gb[ci] + in->c_groups[ci];
    return s2_resident_core(ctx, contigs, n_contigs, P, gb, in->h_gc, in->h_range, nullptr, nullptr, epsilon, out);
}

}  // extern "C"

namespace {

// S2 behind its prologue, for both entries: the re-insertion (S2Plan::run) and the epilogue on the device.  The input groups are numbered contig-major (gb: the first
// group of every contig; in_contig, in_range per group); their id windows are the plan's (from the lists) or computed from the plan's source handle.
int s2_resident_core(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, S2Plan& P, const std::vector<uint64_t>& gb,
                     const std::vector<uint32_t>& in_contig, const std::vector<uint32_t>& in_range, const uint32_t* read_order, const uint64_t* order_off, double epsilon,
                     floria_hip_haplosets** out) {
    const uint32_t n_in = (uint32_t)in_contig.size(), n_groups = n_in;
    std::unique_ptr<floria_hip_haplosets> hs(new (std::nothrow) floria_hip_haplosets);
    if (!hs) return fail(FLORIA_E_NOMEM, "new");
    hs->ctx = ctx; hs->contigs.assign(contigs, contigs + n_contigs); hs->A = P.A;
    hs->c_groups.assign(n_contigs, 0); hs->c_reads.assign(n_contigs, 0);
    if (n_groups == 0) { *out = hs.release(); return 0; }
    Carve C;
    P.carve(C, n_contigs, read_order, order_off);
    const uint32_t tiles_in = (n_in + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
    const Seg s_gb2 = C.seg(8ull * (n_contigs + 1)), s_ic = C.seg(4ull * n_in), s_ir = C.seg(8ull * n_in), s_rl = C.seg(4ull * n_in), s_rh = C.seg(4ull * n_in),
              s_no = C.seg(8ull * (n_in + 1)), s_ko = C.seg(8ull * (n_in + 1)), s_ti = C.seg(8ull * tiles_in + 8), s_cnt = C.seg(16ull * n_contigs);
    int rc = C.place(ctx->misc); if (rc) return rc;
    EventTimer T(ctx->stream);
    if (P.n_assign) { rc = P.run(ctx, contigs, n_contigs, C, T, read_order, order_off, epsilon); if (rc) return rc; }
    else {                                             // no read at all: nothing to re-insert, the groups stay (empty, with their ranges)
        HIPCHK(C.up(P.s_cd, P.cdev.data(), sizeof(fl::ContigDev) * n_contigs, ctx->stream)); HIPCHK(C.up(P.s_ab, P.assign_base.data(), 8ull * n_contigs, ctx->stream));
    }
    int th = T.begin(K_H2D);
    HIPCHK(C.up(s_gb2, gb.data(), 8ull * (n_contigs + 1), ctx->stream)); HIPCHK(C.up(s_ic, in_contig.data(), 4ull * n_in, ctx->stream));
    HIPCHK(C.up(s_ir, in_range.data(), 8ull * n_in, ctx->stream));
    if (!P.src) { HIPCHK(C.up(s_rl, P.rid_lo.data(), 4ull * n_in, ctx->stream)); HIPCHK(C.up(s_rh, P.rid_hi.data(), 4ull * n_in, ctx->stream)); }
    T.end(th);
    if (P.src) hipLaunchKernelGGL(fl::hp_rid_kernel, dim3(items_grid(ctx, n_in, 256)), dim3(256), 0, ctx->stream, P.src->d_go, P.src->d_gr, n_in, P.src->n_reads, C.at<uint32_t>(s_rl), C.at<uint32_t>(s_rh));
    fl::HsArgs a{};
    a.contigs = C.at<const fl::ContigDev>(P.s_cd); a.assign = C.at<const int32_t>(P.s_as); a.assign_base = C.at<const uint64_t>(P.s_ab);
    a.grp_base = C.at<const uint64_t>(s_gb2); a.in_contig = C.at<const uint32_t>(s_ic); a.in_range = C.at<const uint32_t>(s_ir);
    a.rid_lo = C.at<const uint32_t>(s_rl); a.rid_hi = C.at<const uint32_t>(s_rh); a.new_off = C.at<uint64_t>(s_no); a.kept_off = C.at<uint64_t>(s_ko);
    a.counts = C.at<uint64_t>(s_cnt); a.n_contigs = n_contigs; a.n_in = n_in; a.split = ctx->knobs.s2_assign_only ? 0 : 1;
    const uint32_t grid_in = items_grid(ctx, n_in, 4);
    int tk = T.begin(K_SEL);
    hipLaunchKernelGGL(fl::hs_count_kernel, dim3(grid_in), dim3(256), 0, ctx->stream, a);
    launch_offset_scan(ctx, a.new_off, C.at<uint64_t>(s_ti), n_in);
    launch_offset_scan(ctx, a.kept_off, C.at<uint64_t>(s_ti), n_in);
    hipLaunchKernelGGL(fl::hs_contig_counts_kernel, dim3(items_grid(ctx, n_contigs, 256)), dim3(256), 0, ctx->stream, a);
    T.end(tk);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> counts(2ull * n_contigs);
    int td = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(counts.data(), a.counts, 16ull * n_contigs, hipMemcpyDeviceToHost, ctx->stream));      // the call's one copy back: two words per contig
    T.end(td);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint64_t NG = 0, NR = 0;
    for (uint32_t ci = 0; ci < n_contigs; ++ci) { hs->c_groups[ci] = counts[2 * ci]; hs->c_reads[ci] = counts[2 * ci + 1]; NG += counts[2 * ci]; NR += counts[2 * ci + 1]; }
    if (NG < n_in || NR > P.n_assign) return fail(FLORIA_E_DEVICE, "reassign_batch_resident: the device's group counts are inconsistent");
    if (NG >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "reassign_batch_resident: 2^32 and more haplosets in one call");
    hs->n_groups = NG; hs->n_reads = NR;
    Carve H;                                           // the handle's own buffer
    HsSegs hseg; std::vector<fl::SpanContig> sc;
    rc = hs_place(hs.get(), contigs, n_contigs, NG, NR, H, hseg, sc); if (rc) return rc;
    Carve S;                                           // the slot tables between the kernels
    const uint32_t tiles_out = (uint32_t)((NG + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE);
    const Seg s_sa = S.seg(4 * NG), s_sb = S.seg(4 * NG), s_sr = S.seg(8 * NG), s_sd = S.seg(4 * NG), s_to = S.seg(8ull * tiles_out + 8);
    rc = S.place(ctx->hs_tmp); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(H.at(hseg.cd), C.at(P.s_cd), sizeof(fl::ContigDev) * n_contigs, hipMemcpyDeviceToDevice, ctx->stream));
    a.slot_a = S.at<uint32_t>(s_sa); a.slot_b = S.at<uint32_t>(s_sb); a.slot_range = S.at<uint32_t>(s_sr); a.slot_dst = S.at<uint32_t>(s_sd);
    a.grp_contig = H.at<uint32_t>(hseg.gc); a.grp_off = H.at<uint64_t>(hseg.go); a.grp_read = H.at<uint32_t>(hseg.gr); a.range = H.at<uint32_t>(hseg.rg);
    a.n_out = NG; a.n_reads_out = NR;
    tk = T.begin(K_SEL);
    hipLaunchKernelGGL(fl::hs_slots_kernel, dim3(grid_in), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(fl::hs_rank_kernel, dim3(items_grid(ctx, NG, 256)), dim3(256), 0, ctx->stream, a);
    launch_offset_scan(ctx, a.grp_off, S.at<uint64_t>(s_to), (uint32_t)NG);
    hipLaunchKernelGGL(fl::hs_fill_kernel, dim3(grid_in), dim3(256), 0, ctx->stream, a);
    T.end(tk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    T.publish(ctx->timing);
    *out = hs.release();
    return 0;
}

}  // namespace

extern "C" {

void floria_hip_haplosets_free(floria_hip_haplosets* hs) {
    if (!hs) return;
    (void)hipSetDevice(hs->ctx->device);
    delete hs;
}

int floria_hip_haplosets_download(const floria_hip_haplosets* hs, floria_groups*** out) {
    if (!hs || !out) return fail(FLORIA_E_INVALID, "null argument");
    *out = nullptr;
    if (int rc = hs_headers(hs)) return rc;
    const uint32_t n_contigs = (uint32_t)hs->contigs.size();
    std::vector<uint32_t> reads(hs->n_reads + 1);
    if (hs->n_reads) {
        HIPCHK(hipSetDevice(hs->ctx->device));
        HIPCHK(hipMemcpyAsync(reads.data(), hs->d_gr, 4 * hs->n_reads, hipMemcpyDeviceToHost, hs->ctx->stream));
        HIPCHK(hipStreamSynchronize(hs->ctx->stream));
    }
    floria_groups** arr = (floria_groups**)calloc(std::max(1u, n_contigs), sizeof(floria_groups*));
    if (!arr) return fail(FLORIA_E_NOMEM, "calloc");
    uint64_t g0 = 0;
    for (uint32_t ci = 0; ci < n_contigs; ++ci) {
        const uint64_t ng = hs->c_groups[ci], r0 = hs->h_off[g0], tot = hs->h_off[g0 + ng] - r0;
        floria_groups* G = (floria_groups*)calloc(1, sizeof(floria_groups));
        if (G) { G->grp_off = (uint64_t*)calloc(ng + 1, 8); G->range = (uint32_t*)calloc(2 * ng + 2, 4); G->grp_read = (uint32_t*)malloc(4 * (tot + 1)); }
        arr[ci] = G;
        if (!G || !G->grp_off || !G->range || !G->grp_read) { floria_hip_groups_array_free(arr, n_contigs); return fail(FLORIA_E_NOMEM, "calloc"); }
        G->n_groups = (uint32_t)ng;
        for (uint64_t k = 0; k <= ng; ++k) G->grp_off[k] = hs->h_off[g0 + k] - r0;
        std::copy(hs->h_range.begin() + 2 * g0, hs->h_range.begin() + 2 * (g0 + ng), G->range);
        std::copy(reads.begin() + r0, reads.begin() + r0 + tot, G->grp_read);
        g0 += ng;
    }
    *out = arr;
    return 0;
}

int floria_hip_haploset_stats_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs, double* out4) {
    if (int rc = hs_check(ctx, contigs, n_contigs, hs, "haploset_stats_resident")) return rc;
    if (hs->n_groups && !out4) return fail(FLORIA_E_INVALID, "null argument");
    if (hs->n_groups == 0) return 0;
    if (int rc = hs_headers(hs)) return rc;
    return stats_core(ctx, hs->A, hs->h_range.data(), (uint32_t)hs->n_groups, nullptr, hs_dev(hs, false), out4);
}

int floria_hip_haploset_alleles_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs,
                                         const uint64_t* pos_off, uint32_t* counts) {
    if (int rc = hs_check(ctx, contigs, n_contigs, hs, "haploset_alleles_resident")) return rc;
    if (hs->n_groups && !pos_off) return fail(FLORIA_E_INVALID, "null argument");
    if (hs->n_groups == 0) return 0;
    if (int rc = hs_headers(hs)) return rc;
    return alleles_core(ctx, hs->h_range.data(), (uint32_t)hs->n_groups, pos_off, nullptr, hs_dev(hs, false), counts);
}

int floria_hip_read_spans_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs,
                                   uint32_t* left, uint32_t* right) {
    if (int rc = hs_check(ctx, contigs, n_contigs, hs, "read_spans_resident")) return rc;
    for (uint32_t i = 0; i < n_contigs; ++i) if (!contigs[i]->seq_pos) return fail(FLORIA_E_INVALID, "the contig carries no seq_pos");
    if (hs->n_groups == 0 || hs->n_reads == 0) return 0;
    if (!left || !right) return fail(FLORIA_E_INVALID, "null argument");
    return spans_core(ctx, n_contigs, hs->n_reads, (uint32_t)hs->n_groups, nullptr, hs_dev(hs, true), left, right);
}

int floria_hip_hapq_batch_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* chs,
                                   const uint64_t* const* snp_to_genome_pos, const uint32_t* n_snps, uint64_t block_length,
                                   uint8_t* hapq, double* rel_err, double* avg_err) {
    if (int rc = hs_check(ctx, contigs, n_contigs, chs, "hapq_batch_resident")) return rc;
    if ((n_contigs && !avg_err) || (chs->n_groups && (!hapq || !rel_err))) return fail(FLORIA_E_INVALID, "null argument");
    if (block_length == 0) return fail(FLORIA_E_INVALID, "block_length must be positive");
    for (uint32_t c = 0; c < n_contigs; ++c) avg_err[c] = std::numeric_limits<double>::quiet_NaN();
    if (chs->n_groups == 0) return 0;
    floria_hip_haplosets* hs = const_cast<floria_hip_haplosets*>(chs);
    const uint32_t n_groups = (uint32_t)hs->n_groups;
    if (int rc = hs_headers(hs)) return rc;
    std::vector<double> st(4ull * n_groups);
    if (int rc = stats_core(ctx, hs->A, hs->h_range.data(), n_groups, nullptr, hs_dev(hs, false), st.data())) return rc;
    if (int rc = hs_spans(ctx, hs)) return rc;
    return hapq_core(ctx, contigs, n_contigs, hs->h_gc, hs->h_off.data(), hs->h_range.data(), n_groups, st, hs->h_lo, hs->h_len, snp_to_genome_pos, n_snps, block_length,
                     nullptr, hs_dev(hs, false), hapq, rel_err, avg_err);
}

// ---- hap-graph paths -> haplosets on the resident S1 batch (path_kernel.h) -----------------------------------------------------------------------------------------
int floria_hip_join_paths(floria_hip_ctx* ctx, const floria_block_result* res, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                          const uint32_t* path_contig, const uint64_t* node_off, const uint32_t* node_block, const uint8_t* node_part,
                          const uint32_t* path_range, uint32_t n_paths, floria_hip_haplosets** out) {
    if (!ctx) return fail(FLORIA_E_INVALID, "join_paths: null argument (ctx)");
    if (!res) return fail(FLORIA_E_INVALID, "join_paths: null argument (res)");
    if (!out) return fail(FLORIA_E_INVALID, "join_paths: null argument (out)");
    *out = nullptr;
    if (n_contigs && !contigs) return fail(FLORIA_E_INVALID, "join_paths: null argument (contigs)");
    if (!node_off) return fail(FLORIA_E_INVALID, "join_paths: null argument (node_off)");
    if (n_paths && !path_contig) return fail(FLORIA_E_INVALID, "join_paths: null argument (path_contig)");
    if (n_paths && !path_range) return fail(FLORIA_E_INVALID, "join_paths: null argument (path_range)");
    if (!ctx->batch_token || res->batch_token != ctx->batch_token) return fail(FLORIA_E_INVALID, "the batch is no longer resident: call floria_hip_hap_graph directly after phase_blocks");
    const uint32_t nb = (uint32_t)ctx->last_bc.size();
    if (res->n_blocks != nb || (nb && !res->best_ploidy)) return fail(FLORIA_E_INVALID, "join_paths: res is not the result of the resident batch");
    for (uint32_t i = 0; i < n_contigs; ++i) {
        if (!contigs[i]) return fail(FLORIA_E_INVALID, "join_paths: null argument (contigs[" + std::to_string(i) + "])");
        if (contigs[i]->ctx != ctx) return fail(FLORIA_E_INVALID, "join_paths: contig " + std::to_string(i) + " belongs to another context");
    }
    if (n_contigs != ctx->last_contigs.size()) return fail(FLORIA_E_INVALID, "join_paths: contigs: " + std::to_string(n_contigs) + " given, the S1 call had " + std::to_string(ctx->last_contigs.size()));
    for (uint32_t i = 0; i < n_contigs; ++i)
        if (contigs[i] != ctx->last_contigs[i]) return fail(FLORIA_E_INVALID, "join_paths: contigs[" + std::to_string(i) + "] is not the S1 call's");
    if (node_off[0] != 0) return fail(FLORIA_E_INVALID, "join_paths: node_off does not start at 0");
    for (uint32_t p = 0; p < n_paths; ++p) {
        if (path_contig[p] >= n_contigs) return fail(FLORIA_E_INVALID, "join_paths: path_contig[" + std::to_string(p) + "] out of range");
        if (p && path_contig[p] < path_contig[p - 1]) return fail(FLORIA_E_INVALID, "join_paths: path_contig descends at path " + std::to_string(p));
        if (node_off[p + 1] < node_off[p]) return fail(FLORIA_E_INVALID, "join_paths: node_off descends at path " + std::to_string(p));
    }
    const uint64_t n_nodes = node_off[n_paths];
    if (n_nodes >= (1ull << 32)) return fail(FLORIA_E_UNSUPPORTED, "join_paths: 2^32 and more nodes in one call");
    if (n_nodes && !node_block) return fail(FLORIA_E_INVALID, "join_paths: null argument (node_block)");
    if (n_nodes && !node_part) return fail(FLORIA_E_INVALID, "join_paths: null argument (node_part)");
    std::vector<uint32_t> node_path(n_nodes);
    for (uint32_t p = 0; p < n_paths; ++p)
        for (uint64_t n = node_off[p]; n < node_off[p + 1]; ++n) {
            const uint32_t b = node_block[n];
            if (b >= nb) return fail(FLORIA_E_INVALID, "join_paths: node_block[" + std::to_string(n) + "] out of range");
            if (node_part[n] >= res->best_ploidy[b]) return fail(FLORIA_E_INVALID, "join_paths: node_part[" + std::to_string(n) + "] is not below the best ploidy of block " + std::to_string(b));
            if (ctx->last_bc[b] != path_contig[p]) return fail(FLORIA_E_INVALID, "join_paths: node_block[" + std::to_string(n) + "] belongs to another contig than path " + std::to_string(p));
            node_path[n] = p;
        }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->timing = floria_timing{};
    std::unique_ptr<floria_hip_haplosets> hs(new (std::nothrow) floria_hip_haplosets);
    if (!hs) return fail(FLORIA_E_NOMEM, "new");
    hs->ctx = ctx; hs->contigs.assign(contigs, contigs + n_contigs);
    hs->c_groups.assign(n_contigs, 0); hs->c_reads.assign(n_contigs, 0);
    std::vector<fl::ContigDev> cdev(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) { hs->A = std::max(hs->A, contigs[i]->n_alleles); cdev[i] = contigs[i]->dev; }
    if (n_paths == 0) { *out = hs.release(); return 0; }
    std::vector<uint64_t> pb(n_contigs + 1, 0);
    for (uint32_t p = 0; p < n_paths; ++p) pb[path_contig[p] + 1]++;
    for (uint32_t ci = 0; ci < n_contigs; ++ci) pb[ci + 1] += pb[ci];
    Carve C;                                           // the path tables (the S1 batch lies in misc / misc0 and stays)
    const uint32_t tiles = (n_paths + fl::PILEUP_SCAN_TILE - 1) / fl::PILEUP_SCAN_TILE;
    const Seg s_no = C.seg(8ull * (n_paths + 1)), s_nb = C.seg(4 * n_nodes + 4), s_np = C.seg(n_nodes + 4), s_npa = C.seg(4 * n_nodes + 4), s_pb = C.seg(8ull * (n_contigs + 1)),
              s_wl = C.seg(4ull * n_paths), s_wo = C.seg(8ull * (n_paths + 1)), s_go = C.seg(8ull * (n_paths + 1)), s_ti = C.seg(8ull * tiles + 8), s_cnt = C.seg(16ull * n_contigs);
    int rc = C.place(ctx->hs_tmp); if (rc) return rc;
    EventTimer T(ctx->stream);
    int th = T.begin(K_H2D);
    HIPCHK(C.up(s_no, node_off, 8ull * (n_paths + 1), ctx->stream)); HIPCHK(C.up(s_nb, node_block, 4 * n_nodes, ctx->stream)); HIPCHK(C.up(s_np, node_part, n_nodes, ctx->stream));
    HIPCHK(C.up(s_npa, node_path.data(), 4 * n_nodes, ctx->stream)); HIPCHK(C.up(s_pb, pb.data(), 8ull * (n_contigs + 1), ctx->stream));
    T.end(th);
    fl::PathArgs a{};
    a.bs = ctx->last_bs; a.part = ctx->last_part;
    a.node_off = C.at<const uint64_t>(s_no); a.node_block = C.at<const uint32_t>(s_nb); a.node_part = C.at<const uint8_t>(s_np); a.node_path = C.at<const uint32_t>(s_npa);
    a.path_base = C.at<const uint64_t>(s_pb); a.win_lo = C.at<uint32_t>(s_wl); a.word_off = C.at<uint64_t>(s_wo); a.grp_off = C.at<uint64_t>(s_go); a.counts = C.at<uint64_t>(s_cnt);
    a.n_nodes = n_nodes; a.n_paths = n_paths; a.n_contigs = n_contigs;
    const uint32_t grid_p = items_grid(ctx, n_paths, 4);
    int tk = T.begin(K_SEL);
    hipLaunchKernelGGL(fl::path_window_kernel, dim3(grid_p), dim3(256), 0, ctx->stream, a);
    launch_offset_scan(ctx, a.word_off, C.at<uint64_t>(s_ti), n_paths);
    T.end(tk);
    HIPCHK(hipGetLastError());
    uint64_t n_words = 0;                              // the bitmap's size: 8 B come back before it can be placed
    int td = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(&n_words, a.word_off + n_paths, 8, hipMemcpyDeviceToHost, ctx->stream));
    T.end(td);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n_words > ((uint64_t)n_paths << 26)) return fail(FLORIA_E_DEVICE, "join_paths: the device's window sizes are inconsistent");
    rc = ctx->join_bits.ensure(8 * n_words + 8); if (rc) return rc;
    a.bitmap = ctx->join_bits.as<uint64_t>(); a.n_words = n_words;
    HIPCHK(hipMemsetAsync(a.bitmap, 0, 8 * n_words + 8, ctx->stream));
    tk = T.begin(K_SEL);
    if (n_nodes) hipLaunchKernelGGL(fl::path_mark_kernel, dim3(items_grid(ctx, n_nodes, 4)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(fl::path_count_kernel, dim3(grid_p), dim3(256), 0, ctx->stream, a);
    launch_offset_scan(ctx, a.grp_off, C.at<uint64_t>(s_ti), n_paths);
    hipLaunchKernelGGL(fl::path_contig_counts_kernel, dim3(items_grid(ctx, n_contigs, 256)), dim3(256), 0, ctx->stream, a);
    T.end(tk);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> counts(2ull * n_contigs);
    td = T.begin(K_D2H);
    HIPCHK(hipMemcpyAsync(counts.data(), a.counts, 16ull * n_contigs, hipMemcpyDeviceToHost, ctx->stream));      // two words per contig, as in S2's epilogue
    T.end(td);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint64_t NG = 0, NR = 0;
    for (uint32_t ci = 0; ci < n_contigs; ++ci) { hs->c_groups[ci] = counts[2 * ci]; hs->c_reads[ci] = counts[2 * ci + 1]; NG += counts[2 * ci]; NR += counts[2 * ci + 1]; }
    if (NG != n_paths || NR > 64 * n_words) return fail(FLORIA_E_DEVICE, "join_paths: the device's group counts are inconsistent");
    hs->n_groups = NG; hs->n_reads = NR;
    Carve H;
    HsSegs hseg; std::vector<fl::SpanContig> sc;
    rc = hs_place(hs.get(), contigs, n_contigs, NG, NR, H, hseg, sc); if (rc) return rc;
    th = T.begin(K_H2D);
    HIPCHK(H.up(hseg.cd, cdev.data(), sizeof(fl::ContigDev) * n_contigs, ctx->stream)); HIPCHK(H.up(hseg.gc, path_contig, 4ull * n_paths, ctx->stream));
    HIPCHK(H.up(hseg.rg, path_range, 8ull * n_paths, ctx->stream));
    T.end(th);
    HIPCHK(hipMemcpyAsync(H.at(hseg.go), a.grp_off, 8ull * (n_paths + 1), hipMemcpyDeviceToDevice, ctx->stream));
    a.grp_read = H.at<uint32_t>(hseg.gr); a.n_reads_out = NR;
    tk = T.begin(K_SEL);
    hipLaunchKernelGGL(fl::path_fill_kernel, dim3(grid_p), dim3(256), 0, ctx->stream, a);
    T.end(tk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    T.publish(ctx->timing);
    *out = hs.release();
    return 0;
}

}  // extern "C"
