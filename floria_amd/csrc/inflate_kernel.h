// inflate_kernel.h — BGZF members inflated on the device (floria_hip_inflate_bgzf) and the record table of the inflated bytes (floria_hip_blob_records, floria_hip_blob_records_opt).
//
// ONE DECODER TEXT.  inflate_core is raw DEFLATE (RFC 1951: stored, fixed and dynamic blocks, any number of blocks) as one __host__ __device__ function template
// over three memory accessors, so the text the GPU runs also compiles for the CPU (tests/cpp/inflate_core_check.cpp runs it under the sanitizers against zlib):
//   In   word(i)  little-endian 32-bit word i of the payload, bytes at and behind the payload's length read as 0;  byte(i)  payload byte i (0 behind the end)
//   Out  put(pos, b)  one literal;  copy(pos, dist, len)  a match: out[pos + i] = out[pos - dist + i % dist], i < len (what the overlapping byte copy of the
//        format produces; every source byte lies before pos);  copy_in(pos, in, off, len)  a stored block's bytes
//   Tab  get(i) / set(i, v)  INF_TAB_WORDS 16-bit words: the Huffman tables
// BOUNDS are part of the definition: every input read is bounded by the payload length (the bit reader counts the bits it hands out against 8 x payload and the
// accessors return 0 behind the end), every output write by out_bytes (checked before put / copy / copy_in), every table index by its table (symbols are
// compared with the symbol count, lengths are masked to 0..15, fast-table indices to INF_FAST_BITS bits).  Every trip of every decoding loop consumes at least
// one input bit or emits at least one output byte, so a member ends after at most 8 x payload + out_bytes steps whatever it contains (*steps counts them; the
// table builds between them are loops of constant length).
// Huffman decoding: a direct table over the next INF_FAST_BITS bits (entry = symbol << 4 | length, 0 = no code that short) and, for longer codes, the canonical
// count / symbol walk, one bit per trip.  What zlib's inflate accepts is accepted: an incomplete length or distance code only when its longest code has one bit,
// a distance code without any code, no incomplete code-length code.
//
// THE KERNEL.  One wavefront (a 64-thread workgroup) per member, in a persistent grid over the member list.  All 64 lanes run inflate_core on the same values —
// the control flow is uniform — so the accessors can work for the wave: the payload is fetched 256 B at a time, one aligned word pair per lane, and handed out by
// a lane read; the member's output (at most 64 KiB) and the tables live in LDS; a literal is one lane's byte store; a match is copied by the lanes together, every
// lane computing its source index from bytes that were complete before the match began, so the copy is LDS reads in program order behind one workgroup barrier and
// nothing is read back through global memory; one coalesced flush (aligned 32-bit stores between a byte-wise head and tail) ends the member.  About 68 KiB of LDS
// per wave: two waves per CU.  inflate_crc_kernel then checks the CRC32 of every member's bytes, one lane per member, table-driven from LDS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "common.h"
#define FL_HD __host__ __device__ __forceinline__
#else
#define FL_HD inline
#endif

namespace fl {

// per-member status words (floria_hip_inflate_bgzf names them in its error message)
enum : uint32_t {
    INF_OK = 0,
    INF_BITS_RAN_OUT = 1,      // the payload ended inside a block
    INF_BLOCK_TYPE = 2,        // reserved block type 3
    INF_STORED_LEN = 3,        // LEN / NLEN of a stored block are not complements
    INF_OVERSUBSCRIBED = 4,    // code lengths that over-subscribe the code space
    INF_INCOMPLETE = 5,        // code lengths that leave code space unused (beyond what zlib accepts)
    INF_DISTANCE = 6,          // a distance that reaches before the member's first byte
    INF_TOO_LONG = 7,          // more output than ISIZE
    INF_TOO_SHORT = 8,         // less output than ISIZE
    INF_CRC = 9,               // CRC32 of the output differs from the trailer's
    INF_BAD_CODE = 10,         // a bit pattern or symbol that is no code: length symbols 286 / 287, distance symbols 30 / 31, a repeat without a previous length or
                               // past the last length, more than 286 / 30 symbols, no end-of-block code, a pattern an incomplete code does not assign
    INF_STEPS = 11,            // the step bound was reached (cannot happen: the second line behind the bit and byte counts)
    INF_N_STATUS = 12
};

constexpr uint32_t INF_FAST_BITS = 9, INF_FAST = 1u << INF_FAST_BITS;
constexpr uint32_t INF_MAX_LIT = 288, INF_MAX_DIST = 32, INF_MAX_OUT = 65536;
// table layout in 16-bit words: per code a fast table, counts per length, symbols in canonical order; the code lengths being read; offsets / next codes of a build
constexpr uint32_t T_LFAST = 0, T_DFAST = T_LFAST + INF_FAST, T_LCNT = T_DFAST + INF_FAST, T_LSYM = T_LCNT + 16, T_DCNT = T_LSYM + INF_MAX_LIT, T_DSYM = T_DCNT + 16,
                   T_LENS = T_DSYM + INF_MAX_DIST, T_OFFS = T_LENS + INF_MAX_LIT + INF_MAX_DIST, T_NEXT = T_OFFS + 16, INF_TAB_WORDS = T_NEXT + 16;

// the bit reader: at most 32 bits per request; `used` counts what was handed out, and a request that takes it past 8 x payload fails
template <class In> struct InfBits {
    In& in;
    uint64_t buf = 0, used = 0, total;
    uint32_t cnt = 0, next = 0;
    FL_HD InfBits(In& i, uint32_t in_bytes) : in(i), total(8ull * in_bytes) {}
    FL_HD void refill() { if (cnt <= 32) { buf |= (uint64_t)in.word(next) << cnt; ++next; cnt += 32; } }
    FL_HD uint32_t peek(uint32_t n) { refill(); return (uint32_t)buf & ((1u << n) - 1u); }      // n <= 16
    FL_HD bool drop(uint32_t n) { buf >>= n; cnt -= n; used += n; return used <= total; }       // n <= what a peek left: at least 33 bits
    FL_HD bool bits(uint32_t n, uint32_t& v) { v = peek(n); return drop(n); }
    // a stored block: the reader steps over `bytes` whole bytes from a byte boundary (the caller has checked them against the payload)
    FL_HD void skip_bytes(uint32_t bytes) {
        used += 8ull * bytes;
        next = (uint32_t)(used >> 5);
        const uint32_t r = (uint32_t)used & 31u;
        buf = (uint64_t)in.word(next) >> r; ++next; cnt = 32 - r;
    }
};

FL_HD uint32_t inf_rev(uint32_t c, uint32_t len) {      // the low `len` bits of c, reversed (len 1..15)
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; ++i) { if (i < len) { r = (r << 1) | (c & 1u); c >>= 1; } }
    return r;
}

// canonical Huffman tables of the n code lengths at tab[lens ..]: counts, symbols, fast table.  `codes`: the code-length code, which may not be incomplete.
template <class Tab> FL_HD uint32_t inf_build(Tab& tab, uint32_t lens, uint32_t n, uint32_t t_cnt, uint32_t t_sym, uint32_t t_fast, bool codes) {
    for (uint32_t l = 0; l < 16; ++l) tab.set(t_cnt + l, 0);
    for (uint32_t s = 0; s < n; ++s) { const uint32_t l = tab.get(lens + s) & 15u; tab.set(t_cnt + l, (uint16_t)(tab.get(t_cnt + l) + 1)); }
    int32_t left = 1;
    uint32_t max = 0, off = 0, code = 0;
    tab.set(t_cnt, 0);                                  // symbols without a code are not counted
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = tab.get(t_cnt + l);
        left = left * 2 - (int32_t)c;
        if (left < 0) return INF_OVERSUBSCRIBED;
        if (c) max = l;
        tab.set(T_OFFS + l, (uint16_t)off); off += c;
        code = (code + tab.get(t_cnt + l - 1)) << 1; tab.set(T_NEXT + l, (uint16_t)code);
    }
    if (left > 0 && max != 0 && (codes || max != 1)) return INF_INCOMPLETE;
    for (uint32_t k = 0; k < INF_FAST; ++k) tab.set(t_fast + k, 0);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = tab.get(lens + s) & 15u;
        if (!l) continue;
        const uint32_t o = tab.get(T_OFFS + l), c = tab.get(T_NEXT + l);
        tab.set(T_OFFS + l, (uint16_t)(o + 1)); tab.set(T_NEXT + l, (uint16_t)(c + 1));
        if (o < n) tab.set(t_sym + o, (uint16_t)s);
        if (l <= INF_FAST_BITS) for (uint32_t k = inf_rev(c, l) & (INF_FAST - 1); k < INF_FAST; k += 1u << l) tab.set(t_fast + k, (uint16_t)(s << 4 | l));
    }
    return INF_OK;
}

// one symbol of a code of n symbols
template <class In, class Tab> FL_HD uint32_t inf_decode(InfBits<In>& br, Tab& tab, uint32_t t_cnt, uint32_t t_sym, uint32_t t_fast, uint32_t n, uint32_t& sym) {
    const uint32_t v = br.peek(15);
    const uint32_t e = tab.get(t_fast + (v & (INF_FAST - 1)));
    if (e) { sym = e >> 4; return br.drop(e & 15u) ? INF_OK : INF_BITS_RAN_OUT; }
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; ++len) {
        code |= (int32_t)((v >> (len - 1)) & 1u);
        const int32_t count = tab.get(t_cnt + len);
        if (code - count < first) {
            const uint32_t i = (uint32_t)(index + (code - first));
            if (i >= n) return INF_BAD_CODE;
            sym = tab.get(t_sym + i);
            return br.drop(len) ? INF_OK : INF_BITS_RAN_OUT;
        }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return br.used + 15 > br.total ? INF_BITS_RAN_OUT : INF_BAD_CODE;
}

// position i of the code-length code's transmission order: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
FL_HD uint32_t inf_order(uint32_t i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i < 19 ? i - 12 : 6))) & 31u);
}

// Raw DEFLATE of in_bytes payload bytes into exactly out_bytes output bytes.  Returns an INF_* status; *steps receives the number of decoding steps.
template <class In, class Out, class Tab>
FL_HD uint32_t inflate_core(In& in, uint32_t in_bytes, Out& out, uint32_t out_bytes, Tab& tab, uint64_t* steps_out) {
    InfBits<In> br(in, in_bytes);
    const uint64_t step_cap = 8ull * in_bytes + out_bytes + 8;
    uint64_t steps = 0;
    uint32_t pos = 0, last = 0, st = INF_OK;
    bool fixed_built = false;
    do {
        uint32_t hdr;
        ++steps;
        if (!br.bits(3, hdr)) { st = INF_BITS_RAN_OUT; break; }
        last = hdr & 1u;
        const uint32_t type = hdr >> 1;
        if (type == 3) { st = INF_BLOCK_TYPE; break; }
        if (type == 0) {
            uint32_t len, nlen;
            const uint32_t r = (uint32_t)br.used & 7u;
            if (r) br.drop(8 - r);
            if (!br.bits(16, len) || !br.bits(16, nlen)) { st = INF_BITS_RAN_OUT; break; }
            if ((len ^ nlen) != 0xffffu) { st = INF_STORED_LEN; break; }
            if (br.used + 8ull * len > br.total) { st = INF_BITS_RAN_OUT; break; }
            if (len > out_bytes - pos) { st = INF_TOO_LONG; break; }
            if (len) { out.copy_in(pos, in, (uint32_t)(br.used >> 3), len); pos += len; br.skip_bytes(len); }
            continue;
        }
        uint32_t nl = INF_MAX_LIT, nd = INF_MAX_DIST;
        if (type == 1) {
            if (!fixed_built) {
                for (uint32_t s = 0; s < INF_MAX_LIT; ++s) tab.set(T_LENS + s, (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8));
                for (uint32_t s = 0; s < INF_MAX_DIST; ++s) tab.set(T_LENS + INF_MAX_LIT + s, 5);
                st = inf_build(tab, T_LENS, INF_MAX_LIT, T_LCNT, T_LSYM, T_LFAST, false);
                if (st == INF_OK) st = inf_build(tab, T_LENS + INF_MAX_LIT, INF_MAX_DIST, T_DCNT, T_DSYM, T_DFAST, false);
                if (st != INF_OK) break;
                fixed_built = true;
            }
        } else {
            uint32_t a, b, c;
            fixed_built = false;
            if (!br.bits(5, a) || !br.bits(5, b) || !br.bits(4, c)) { st = INF_BITS_RAN_OUT; break; }
            nl = a + 257; nd = b + 1;
            const uint32_t ncode = c + 4;
            if (nl > 286 || nd > 30) { st = INF_BAD_CODE; break; }
            for (uint32_t i = 0; i < 19; ++i) tab.set(T_LENS + i, 0);
            for (uint32_t i = 0; i < ncode && st == INF_OK; ++i) {
                uint32_t l;
                if (!br.bits(3, l)) st = INF_BITS_RAN_OUT; else tab.set(T_LENS + inf_order(i), (uint16_t)l);
            }
            if (st != INF_OK) break;
            // the code-length code borrows the literal/length code's tables; its own lengths are read before the lengths it decodes overwrite them
            st = inf_build(tab, T_LENS, 19, T_LCNT, T_LSYM, T_LFAST, true);
            if (st != INF_OK) break;
            uint32_t idx = 0;
            const uint32_t want = nl + nd;      // <= 316: inside T_LENS' 320 words; the repeats run from the literal/length lengths into the distance lengths
            while (idx < want) {
                uint32_t sym = 0, rep = 0, len = 0;
                if (++steps > step_cap) { st = INF_STEPS; break; }
                st = inf_decode(br, tab, T_LCNT, T_LSYM, T_LFAST, 19, sym);
                if (st != INF_OK) break;
                if (sym < 16) { tab.set(T_LENS + idx, (uint16_t)sym); ++idx; continue; }
                if (sym == 16) {
                    if (idx == 0) { st = INF_BAD_CODE; break; }
                    len = tab.get(T_LENS + idx - 1);
                    if (!br.bits(2, rep)) { st = INF_BITS_RAN_OUT; break; }
                    rep += 3;
                } else if (sym == 17) { if (!br.bits(3, rep)) { st = INF_BITS_RAN_OUT; break; } rep += 3; }
                else if (sym == 18) { if (!br.bits(7, rep)) { st = INF_BITS_RAN_OUT; break; } rep += 11; }
                else { st = INF_BAD_CODE; break; }
                if (rep > want - idx) { st = INF_BAD_CODE; break; }
                for (uint32_t k = 0; k < rep; ++k) tab.set(T_LENS + idx + k, (uint16_t)len);
                idx += rep;
            }
            if (st != INF_OK) break;
            if (tab.get(T_LENS + 256) == 0) { st = INF_BAD_CODE; break; }
            // (the literal/length code last: it takes over the tables the code-length code borrowed; a build reads T_LENS and writes none of it)
            st = inf_build(tab, T_LENS + nl, nd, T_DCNT, T_DSYM, T_DFAST, false);
            if (st == INF_OK) st = inf_build(tab, T_LENS, nl, T_LCNT, T_LSYM, T_LFAST, false);
            if (st != INF_OK) break;
        }
        for (;;) {
            uint32_t sym = 0;
            if (++steps > step_cap) { st = INF_STEPS; break; }
            st = inf_decode(br, tab, T_LCNT, T_LSYM, T_LFAST, nl, sym);
            if (st != INF_OK) break;
            if (sym < 256) {
                if (pos >= out_bytes) { st = INF_TOO_LONG; break; }
                out.put(pos, (uint8_t)sym); ++pos;
                continue;
            }
            if (sym == 256) break;
            const uint32_t s = sym - 257;
            if (s >= 29) { st = INF_BAD_CODE; break; }
            uint32_t len, dist, x = 0, d = 0;
            if (s < 8) len = 3 + s;
            else if (s == 28) len = 258;
            else { const uint32_t e = (s >> 2) - 1; if (!br.bits(e, x)) { st = INF_BITS_RAN_OUT; break; } len = 3 + ((4 + (s & 3u)) << e) + x; }
            st = inf_decode(br, tab, T_DCNT, T_DSYM, T_DFAST, nd, d);
            if (st != INF_OK) break;
            if (d >= 30) { st = INF_BAD_CODE; break; }
            if (d < 4) dist = 1 + d;
            else { const uint32_t e = (d >> 1) - 1; if (!br.bits(e, x)) { st = INF_BITS_RAN_OUT; break; } dist = 1 + ((2 + (d & 1u)) << e) + x; }
            if (dist > pos) { st = INF_DISTANCE; break; }
            if (len > out_bytes - pos) { st = INF_TOO_LONG; break; }
            out.copy(pos, dist, len); pos += len;
        }
        if (st != INF_OK) break;
    } while (!last && steps <= step_cap);
    if (st == INF_OK && !last) st = INF_STEPS;
    if (st == INF_OK && pos < out_bytes) st = INF_TOO_SHORT;
    if (steps_out) *steps_out = st == INF_OK || st == INF_TOO_SHORT ? steps : steps - 1;      // (the step that failed completed nothing)
    return st;
}

#if defined(__HIPCC__)

constexpr uint32_t INF_LDS_BYTES = INF_MAX_OUT + 2 * INF_TAB_WORDS;      // one member's output and the tables

struct InflateArgs {
    const uint8_t* file;         // the compressed bytes on the device, 4-byte aligned, readable up to file_words * 4
    uint64_t file_words;
    const uint64_t* pay_off;     // [n] offset of member m's DEFLATE payload in `file`
    const uint32_t* pay_bytes;   // [n] its length (both validated against the file's length by the host)
    const uint64_t* out_off;     // [n + 1] prefix sums of ISIZE: member m owns blob[out_off[m], out_off[m + 1]), at most INF_MAX_OUT bytes
    uint8_t* blob;
    uint32_t* status;            // [n]
    uint32_t n_members;
};

// the payload for the wave: 64 words at a time, lane l holding word 64 * chunk + l
struct InfDevIn {
    const uint32_t* w; uint64_t n_words;      // the file as aligned words
    const uint8_t* p;                         // the payload
    uint32_t bytes, shift, lane, chunk, reg;
    uint64_t w0;                              // index of the aligned word that holds the payload's first byte
    __device__ __forceinline__ void load(uint32_t c) {
        const uint64_t i = (uint64_t)c * 64 + lane;
        uint32_t v = 0;
        if (4 * i < bytes) {
            const uint64_t k = w0 + i;
            const uint32_t a = k < n_words ? G(w)[k] : 0u, b = shift && k + 1 < n_words ? G(w)[k + 1] : 0u;
            v = shift ? a >> shift | b << (32 - shift) : a;
            const uint64_t rest = bytes - 4 * i;
            if (rest < 4) v &= (1u << (8 * (uint32_t)rest)) - 1u;
        }
        reg = v; chunk = c;
    }
    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if ((i >> 6) != chunk) load(i >> 6);
        return (uint32_t)__shfl((int)reg, (int)(i & 63u));
    }
    __device__ __forceinline__ uint8_t byte(uint32_t i) const { return i < bytes ? G(p)[i] : (uint8_t)0; }
};

struct InfDevOut {
    uint8_t* s; uint32_t lane;
    __device__ __forceinline__ void put(uint32_t pos, uint8_t b) { if (lane == 0) s[pos & (INF_MAX_OUT - 1)] = b; }
    // every source byte was written before this call: by lane 0's puts or by any lane's part of an earlier copy — the barrier orders those LDS writes before the reads
    __device__ __forceinline__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        __syncthreads();
        for (uint32_t i = lane; i < len; i += 64) {
            const uint32_t k = i < dist ? i : i % dist;
            s[(pos + i) & (INF_MAX_OUT - 1)] = s[(pos - dist + k) & (INF_MAX_OUT - 1)];
        }
    }
    __device__ __forceinline__ void copy_in(uint32_t pos, const InfDevIn& in, uint32_t off, uint32_t len) {
        for (uint32_t i = lane; i < len; i += 64) s[(pos + i) & (INF_MAX_OUT - 1)] = in.byte(off + i);
    }
};

struct InfDevTab {
    uint16_t* t;
    __device__ __forceinline__ uint16_t get(uint32_t i) const { return i < INF_TAB_WORDS ? t[i] : (uint16_t)0; }
    __device__ __forceinline__ void set(uint32_t i, uint16_t v) { if (i < INF_TAB_WORDS) t[i] = v; }      // (all lanes, the same value)
};

__global__ __launch_bounds__(64) void inflate_kernel(InflateArgs g) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint8_t* s_out = smem;
    uint16_t* s_tab = (uint16_t*)(smem + INF_MAX_OUT);
    const uint32_t lane = threadIdx.x;
    for (uint32_t m = blockIdx.x; m < g.n_members; m += gridDim.x) {
        const uint64_t po = g.pay_off[m], oo = g.out_off[m];
        const uint64_t ob64 = g.out_off[m + 1] - oo;
        const uint32_t ob = ob64 > INF_MAX_OUT ? INF_MAX_OUT : (uint32_t)ob64;
        __syncthreads();                                    // the flush of the member before has read s_out
        InfDevIn in{(const uint32_t*)g.file, g.file_words, g.file + po, g.pay_bytes[m], (uint32_t)(po & 3) * 8, lane, 0xffffffffu, 0u, po >> 2};
        InfDevOut out{s_out, lane};
        InfDevTab tab{s_tab};
        uint32_t st = inflate_core(in, in.bytes, out, ob, tab, (uint64_t*)nullptr);
        if (ob64 > INF_MAX_OUT) st = INF_TOO_LONG;          // (the host refuses such a member: the second line)
        __syncthreads();
        if (st == INF_OK) {
            uint8_t* dst = g.blob + oo;
            const uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
            const uint32_t h = head < ob ? head : ob, words = (ob - h) >> 2, tail = h + 4 * words;
            if (lane < h) dst[lane] = s_out[lane];
            uint32_t* d32 = (uint32_t*)(dst + h);
            for (uint32_t i = lane; i < words; i += 64) {
                const uint32_t o = h + 4 * i;
                d32[i] = (uint32_t)s_out[o] | (uint32_t)s_out[o + 1] << 8 | (uint32_t)s_out[o + 2] << 16 | (uint32_t)s_out[o + 3] << 24;
            }
            if (tail + lane < ob) dst[tail + lane] = s_out[tail + lane];
        }
        if (lane == 0) g.status[m] = st;
    }
}

// CRC32 (the gzip polynomial, reflected: 0xEDB88320) of every member's output against its trailer, one lane per member; a member that already has a status keeps it
__global__ __launch_bounds__(256) void inflate_crc_kernel(const uint8_t* blob, const uint64_t* out_off, const uint32_t* crc_want, uint32_t* status, uint32_t n_members) {
    __shared__ uint32_t s_t[256];
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        s_t[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_members || status[m] != INF_OK) return;
    uint64_t b = out_off[m];
    const uint64_t e = out_off[m + 1];
    uint32_t crc = 0xffffffffu;
    while (b < e && (b & 3)) { crc = s_t[(crc ^ G(blob)[b]) & 255u] ^ (crc >> 8); ++b; }
    for (; b + 4 <= e; b += 4) {
        crc ^= *(const __attribute__((address_space(1))) uint32_t*)G(blob + b);      // blob is 256-byte aligned and b a multiple of 4
        crc = s_t[crc & 255u] ^ (crc >> 8); crc = s_t[crc & 255u] ^ (crc >> 8); crc = s_t[crc & 255u] ^ (crc >> 8); crc = s_t[crc & 255u] ^ (crc >> 8);
    }
    for (; b < e; ++b) crc = s_t[(crc ^ G(blob)[b]) & 255u] ^ (crc >> 8);
    if (~crc != crc_want[m]) status[m] = INF_CRC;
}

// ---- the record table of a blob (floria_hip_blob_records) -----------------------------------------------------------------------------------------------------------
enum : uint32_t { CHAIN_OK = 0, CHAIN_SHORT = 1 /* block_size < 32 */, CHAIN_PAST = 2 /* the record, or its block_size prefix, runs past the chain's end */ };
// how a chain may end (floria_hip_blob_records_opt; == FLORIA_CHAIN_*) and how it did end (floria_blob_records::chain_why)
enum : uint32_t { CHAIN_CUT_TAIL = 1, CHAIN_ONE_REF = 2 };
enum : uint32_t { WHY_END = 0 /* reached end[c] exactly */, WHY_CUT = 1 /* a prefix or record cut by end[c] */, WHY_REF = 2 /* a record of another reference */ };

__device__ __forceinline__ uint32_t blob_u16(const uint8_t* p, uint64_t o) { return (uint32_t)G(p)[o] | (uint32_t)G(p)[o + 1] << 8; }
__device__ __forceinline__ uint32_t blob_u32(const uint8_t* p, uint64_t o) { return blob_u16(p, o) | blob_u16(p, o + 2) << 16; }

struct ChainArgs {
    const uint8_t* blob; uint64_t blob_bytes;
    const uint64_t *begin, *end;      // [n_chains], begin <= end <= blob_bytes (the host checked)
    uint64_t* count;                  // [n_chains + 1] COUNT: records of the chain; then their prefix sums
    uint64_t* stop;                   // [n_chains] where the chain stopped
    uint32_t* status;                 // [n_chains]
    uint32_t* why;                    // [n_chains] WHY_*
    uint64_t* rec_off;                // FILL: [n_records] offset of every record's block_size prefix
    uint32_t n_chains;
    uint32_t flags;                   // CHAIN_CUT_TAIL | CHAIN_ONE_REF, the same in COUNT and FILL: both passes stop at the same record
};

// One lane per chain: follow the block_size prefixes while a whole record fits before the chain's end.  Every trip advances by at least 36 bytes.
// CHAIN_CUT_TAIL: a prefix or a record cut by the end stops the chain in front of that prefix without a status.  CHAIN_ONE_REF: the chain stops in front of the
// first record whose refID is not its first record's; the refID is read behind the fit checks, which have shown the record's 32 fixed bytes to lie before `end`.
template <bool FILL> __global__ __launch_bounds__(256) void blob_chain_kernel(ChainArgs g) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.n_chains) return;
    const uint64_t end = g.end[c] < g.blob_bytes ? g.end[c] : g.blob_bytes;
    const bool cut_tail = g.flags & CHAIN_CUT_TAIL, one_ref = g.flags & CHAIN_ONE_REF;
    uint64_t off = g.begin[c], n = 0;
    const uint64_t slot = FILL ? g.count[c] : 0, cap = FILL ? g.count[c + 1] - slot : 0;
    uint32_t st = CHAIN_OK, why = WHY_END, ref0 = 0;
    while (off < end) {
        if (end - off < 4) { if (cut_tail) why = WHY_CUT; else st = CHAIN_PAST; break; }
        const uint32_t bs = blob_u32(g.blob, off);
        if (bs < 32) { st = CHAIN_SHORT; break; }
        if ((uint64_t)bs > end - off - 4) { if (cut_tail) why = WHY_CUT; else st = CHAIN_PAST; break; }
        if (one_ref) {
            const uint32_t ref = blob_u32(g.blob, off + 4);
            if (n == 0) ref0 = ref; else if (ref != ref0) { why = WHY_REF; break; }
        }
        if (FILL) { if (n >= cap) break; g.rec_off[slot + n] = off; }
        ++n; off += 4 + (uint64_t)bs;
    }
    if (!FILL) { g.count[c] = n; g.stop[c] = off; g.status[c] = st; g.why[c] = why; }
}

struct RecordArgs {
    const uint8_t* blob; uint64_t blob_bytes;
    const uint64_t* rec_off;          // [n]
    int32_t *ref_id, *pos; uint32_t *block_size, *l_seq, *cigar0; uint16_t *flag, *n_cigar_op; uint8_t *mapq, *l_read_name;
    uint64_t* name_off;               // [n + 1] COUNT: the name's bytes; then their prefix sums
    uint8_t* names;
    uint64_t n_records;
};

// One thread per record: the fixed fields, the first CIGAR word (0 where the record has none or it does not fit), the length of the name as stored (l_read_name
// bytes, the NUL included, cut at the record's end).  The chain kernel guarantees offset + 36 <= blob_bytes for every record.
__global__ __launch_bounds__(256) void blob_record_kernel(RecordArgs g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n_records) return;
    const uint64_t o = g.rec_off[i];
    if (o > g.blob_bytes || g.blob_bytes - o < 36) { g.name_off[i] = 0; return; }
    const uint32_t bs = blob_u32(g.blob, o), lrn = G(g.blob)[o + 12], nco = blob_u16(g.blob, o + 16);
    const uint64_t rec_end = o + 4 + (uint64_t)bs <= g.blob_bytes ? o + 4 + (uint64_t)bs : g.blob_bytes;
    g.block_size[i] = bs;
    g.ref_id[i] = (int32_t)blob_u32(g.blob, o + 4); g.pos[i] = (int32_t)blob_u32(g.blob, o + 8);
    g.l_read_name[i] = (uint8_t)lrn; g.mapq[i] = G(g.blob)[o + 13];
    g.n_cigar_op[i] = (uint16_t)nco; g.flag[i] = (uint16_t)blob_u16(g.blob, o + 18);
    g.l_seq[i] = blob_u32(g.blob, o + 20);
    const uint64_t cg = o + 36 + lrn;
    g.cigar0[i] = nco && cg + 4 <= rec_end ? blob_u32(g.blob, cg) : 0u;
    g.name_off[i] = o + 36 + lrn <= rec_end ? lrn : rec_end > o + 36 ? rec_end - (o + 36) : 0;
}

__global__ __launch_bounds__(256) void blob_names_kernel(RecordArgs g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n_records) return;
    const uint64_t o = g.rec_off[i] + 36, b = g.name_off[i], n = g.name_off[i + 1] - b;
    if (n > 255 || o > g.blob_bytes || g.blob_bytes - o < n) return;
    for (uint64_t k = 0; k < n; ++k) g.names[b + k] = G(g.blob)[o + k];
}

#endif  // __HIPCC__

}  // namespace fl
