// ingest.cpp — BAM / VCF / FASTA -> Frags (file_reader.rs), from scratch on zlib: the reference links htslib, which this image
// does not have.  What is restated:
//   get_contigs_to_phase           file_reader.rs:738-746   BAM header target names
//   get_vcf_profile (+ get_genotypes_from_vcf_hts)   :113-175, :239-314   SNP filter: every allele one character of ACGT (any case)
//   alignment_passed_check         :179-235
//   frag_from_record               :661-736   CIGAR walk (rust-htslib aligned_pairs_full), allele = index of the read base in the
//                                             record's allele list, qual = base quality
//   combine_frags                  :491-659   pair merge, supplementary merge with the distance cutoff
//   get_frags_from_bamvcf_rewrite  :343-460   (frags with SNPs, frags without)
//   get_fasta_seqs                 :462-489   whole sequences (the writers need the contig length)
//   l_epsilon_auto_detect          :749-826   every 1000th pileup column: minority / majority base ratio, read-length quantile
//   alignment::realign             alignment.rs:7-64   around every called SNP the read's 32 bases are globally aligned to the reference's 32
//                                  bases with each allele in turn (match +1, mismatch -1, gap open -2, extend -1) and the best-scoring
//                                  allele replaces the call.  The reference computes the scores with block-aligner 0.4.0 (a third-party
//                                  adaptive banded SIMD aligner, fixed 8-wide blocks); here they come from the exact affine-gap DP, which
//                                  the banded heuristic approximates — identical wherever its band contains an optimal path (parity of this
//                                  step is unpinned: third-party arithmetic).  Only runs when a reference FASTA is given, as in the reference.
// Without an index the whole BAM is read once and records are bucketed by contig in file order; with a .bai beside it only the contigs selected for phasing
// are read, each from its indexed offset (BamStream::select; read_bai: SAM specification 5.2).  Either way `count` (the enumerate
// index frag_from_record stores in counter_id, which breaks ties of Frag::cmp in all_frags.sort(), floria.rs:289) is the
// record's index among the contig's records, as with the reference's fetch().
#include "floria_host.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>
#include <thread>
#include <type_traits>
#include <unordered_map>

namespace floria {

namespace {

std::vector<unsigned char> slurp(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw Error(FLORIA_E_INVALID, "cannot open " + path);
    std::vector<unsigned char> buf;
    if (fseek(f, 0, SEEK_END) == 0) { const long n = ftell(f); if (n > 0) buf.reserve((size_t)n); }
    rewind(f);
    unsigned char chunk[1 << 16];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
    fclose(f);
    return buf;
}

// one task per index on up to `threads` threads (first exception rethrown on the caller)
template <class F> void parallel_tasks(size_t n, size_t threads, F&& f) {
    threads = std::min(threads, n);
    if (threads <= 1) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    std::vector<std::thread> pool;
    for (size_t t = 0; t < threads; ++t)
        pool.emplace_back([&] {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= n) return;
                try { f(i); } catch (...) { std::lock_guard<std::mutex> g(mu); if (!err) err = std::current_exception(); next = n; return; }
            }
        });
    for (std::thread& t : pool) t.join();
    if (err) std::rethrow_exception(err);
}

// BGZF members carry their compressed size (extra subfield 'B','C') and end with ISIZE, so their places in the output are known
// before any is inflated: -> false if `in` is not made of BGZF members only (plain gzip: the serial path takes it)
struct BgzfBlock { size_t in_off, in_len, out_off, out_len; };
struct ByteSpan { const unsigned char* p; size_t n; size_t size() const { return n; } const unsigned char& operator[](size_t i) const { return p[i]; } };
// the header of the member that starts at in[o]: its compressed size and the inflated size its last four bytes give; false: no BGZF member starts there
bool bgzf_member(const ByteSpan& in, size_t o, size_t& bsize, uint32_t& isize) {
    if (o + 18 > in.size() || in[o] != 0x1f || in[o + 1] != 0x8b || in[o + 2] != 8 || !(in[o + 3] & 4)) return false;
    const size_t xlen = in[o + 10] | (in[o + 11] << 8);
    if (o + 12 + xlen > in.size()) return false;
    size_t x = o + 12;
    bsize = 0;
    while (x + 4 <= o + 12 + xlen) {
        const size_t slen = in[x + 2] | (in[x + 3] << 8);
        if (in[x] == 'B' && in[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) bsize = (size_t)(in[x + 4] | (in[x + 5] << 8)) + 1;
        x += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || o + bsize > in.size()) return false;
    memcpy(&isize, &in[o + bsize - 4], 4);
    return true;
}
bool bgzf_index(const ByteSpan& in, std::vector<BgzfBlock>& blocks) {
    size_t o = 0, out = 0;
    while (o < in.size()) {
        size_t bsize; uint32_t isize;
        if (!bgzf_member(in, o, bsize, isize)) return false;
        blocks.push_back({o, bsize, out, isize});
        o += bsize; out += isize;
    }
    return true;
}

// BGZF = concatenated gzip members; inflate them all
std::vector<unsigned char> bgzf_inflate_all(const std::vector<unsigned char>& in, const std::string& what, size_t threads) {
    std::vector<unsigned char> out;
    std::vector<BgzfBlock> blocks;
    if (threads > 1 && bgzf_index(ByteSpan{in.data(), in.size()}, blocks)) {
        out.resize(blocks.empty() ? 0 : blocks.back().out_off + blocks.back().out_len);
        const size_t per = 64;                                                     // members per task
        parallel_tasks((blocks.size() + per - 1) / per, threads, [&](size_t t) {
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) throw Error(FLORIA_E_NOMEM, "inflateInit2 failed");
            for (size_t b = t * per; b < std::min(blocks.size(), (t + 1) * per); ++b) {
                const BgzfBlock& k = blocks[b];
                zs.next_in = const_cast<unsigned char*>(in.data()) + k.in_off; zs.avail_in = (uInt)k.in_len;
                unsigned char dummy;
                zs.next_out = k.out_len ? out.data() + k.out_off : &dummy; zs.avail_out = (uInt)k.out_len;
                const int rc = inflate(&zs, Z_FINISH);
                if (rc != Z_STREAM_END || zs.avail_out != 0) { inflateEnd(&zs); throw Error(FLORIA_E_INVALID, what + " is not a valid BGZF/gzip file"); }
                inflateReset(&zs);
            }
            inflateEnd(&zs);
        });
        return out;
    }
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) throw Error(FLORIA_E_NOMEM, "inflateInit2 failed");
    zs.next_in = const_cast<unsigned char*>(in.data());
    zs.avail_in = (uInt)std::min<size_t>(in.size(), 0x7fffffffu);
    size_t consumed_total = 0;
    std::vector<unsigned char> buf(1 << 20);
    while (consumed_total < in.size()) {
        zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
        const unsigned char* before = zs.next_in;
        const int rc = inflate(&zs, Z_NO_FLUSH);
        consumed_total += (size_t)(zs.next_in - before);
        out.insert(out.end(), buf.data(), buf.data() + (buf.size() - zs.avail_out));
        if (rc == Z_STREAM_END) {
            if (consumed_total >= in.size()) break;
            inflateReset(&zs);
            zs.next_in = const_cast<unsigned char*>(in.data()) + consumed_total;
            zs.avail_in = (uInt)std::min<size_t>(in.size() - consumed_total, 0x7fffffffu);
        } else if (rc != Z_OK) { inflateEnd(&zs); throw Error(FLORIA_E_INVALID, what + " is not a valid BGZF/gzip file"); }
        else if (zs.avail_in == 0 && consumed_total < in.size()) {
            zs.next_in = const_cast<unsigned char*>(in.data()) + consumed_total;
            zs.avail_in = (uInt)std::min<size_t>(in.size() - consumed_total, 0x7fffffffu);
        }
    }
    inflateEnd(&zs);
    return out;
}

struct Cursor {
    const unsigned char* p; size_t n, o = 0;
    const std::string& what;
    void need(size_t k) const { if (o + k > n) throw Error(FLORIA_E_INVALID, what + " is truncated"); }
    uint32_t u32() { need(4); uint32_t v; memcpy(&v, p + o, 4); o += 4; return v; }
    uint64_t u64() { need(8); uint64_t v; memcpy(&v, p + o, 8); o += 8; return v; }
    int32_t i32() { return (int32_t)u32(); }
    uint16_t u16() { need(2); uint16_t v; memcpy(&v, p + o, 2); o += 2; return v; }
    uint8_t u8() { need(1); return p[o++]; }
};

constexpr uint16_t F_PAIRED1 = 64, F_PAIRED2 = 128, F_SECONDARY = 256, F_SUPP = 2048, F_ERRORS = 1796;

// alignment_passed_check (file_reader.rs:179-235) -> (passed, is_supp)
std::pair<bool, bool> alignment_passed_check(uint16_t flags, uint8_t mapq, bool use_supplementary, bool filter_supplementary, uint8_t mapq_cutoff) {
    const bool is_paired = (flags & F_PAIRED1) || (flags & F_PAIRED2);
    bool is_supp = false;
    if (flags & F_SUPP) {
        is_supp = true;
        if (is_paired) return {false, true};
        if (!use_supplementary) return {false, true};
        if (filter_supplementary && mapq < 60) return {false, true};
    }
    if (mapq < mapq_cutoff) return {false, is_supp};
    if (flags & F_ERRORS) return {false, is_supp};
    if (flags & F_SECONDARY) return {false, is_supp};
    return {true, is_supp};
}

inline int cig_op(uint32_t c) { return (int)(c & 15); }
inline uint32_t cig_len(uint32_t c) { return c >> 4; }
// M I D N S H P = X  ->  consumes query / reference
inline bool consumes_q(int op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
inline bool consumes_r(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

int64_t reference_end(const BamRecord& r) {                 // bam_endpos
    int64_t len = 0;
    for (size_t k = 0; k < r.cigar.size(); ++k) { const uint32_t c = r.cigar[k]; if (consumes_r(cig_op(c))) len += cig_len(c); }
    return (int64_t)r.pos + (len ? len : 1);
}

// the parts of frag_from_record that do not depend on the SNPs: identity and start before the calls, the read's own bases behind them (:728-734)
Frag frag_without_calls(const BamRecord& rec, size_t counter_id) {
    Frag frag;
    frag.id = std::string(rec.qname); frag.counter_id = counter_id;
    frag.is_paired = (rec.flags & F_PAIRED1) || (rec.flags & F_PAIRED2);
    frag.first_position = UINT32_MAX; frag.last_position = 0;
    frag.first_pos_base = (GnPosition)rec.pos;
    return frag;
}
void frag_sequences(Frag& frag, const BamRecord& rec, bool keep_sequences);

// --pileup device: the Frag of a record from the cells floria_hip_pileup_records walked for it (no CIGAR walk, no lookup in the SNP maps)
Frag frag_from_cells(const BamRecord& rec, const RecordPileup::Cells& cells, size_t counter_id, bool keep_sequences) {
    Frag frag = frag_without_calls(rec, counter_id);
    frag.last_pos_base = (GnPosition)cells.ref_end;
    for (size_t k = 0; k < cells.n; ++k) {                                         // (ascending SNPs: every insert appends)
        const SnpPosition snp_pos = cells.snp[k];
        frag.seq_dict[snp_pos] = (Genotype)cells.allele[k];
        frag.qual_dict[snp_pos] = cells.qual[k];
        frag.snp_pos_to_seq_pos[snp_pos] = {0, (GnPosition)cells.seq_pos[k]};
    }
    if (cells.n) { frag.first_position = cells.snp[0]; frag.last_position = cells.snp[cells.n - 1]; }
    frag_sequences(frag, rec, keep_sequences);
    return frag;
}

// frag_from_record (file_reader.rs:661-736)
Frag frag_from_record(const BamRecord& rec, const std::map<GnPosition, SnpPosition>& snp_positions, const std::map<GnPosition, std::vector<Genotype>>& pos_allele_map, size_t counter_id,
                      bool keep_sequences) {
    Frag frag = frag_without_calls(rec, counter_id);
    size_t leading_hardclips = 0;
    if ((rec.flags & F_SUPP) && !rec.cigar.empty() && cig_op(rec.cigar[0]) == 5) leading_hardclips = cig_len(rec.cigar[0]);
    frag.last_pos_base = (GnPosition)reference_end(rec);
    size_t q = 0;
    int64_t r = rec.pos;
    // the SNPs of the contig the alignment spans: walk them together with the CIGAR (positions ascend in both)
    auto snp_it = snp_positions.lower_bound((GnPosition)std::max<int64_t>(0, r));
    for (size_t ck = 0; ck < rec.cigar.size(); ++ck) {
        const uint32_t c = rec.cigar[ck];
        const int op = cig_op(c);
        const uint32_t len = cig_len(c);
        if (op == 0 || op == 7 || op == 8) {                                   // aligned pairs (Some(q), Some(r))
            while (snp_it != snp_positions.end() && (int64_t)snp_it->first < r) ++snp_it;
            while (snp_it != snp_positions.end() && (int64_t)snp_it->first < r + (int64_t)len) {
                const GnPosition genome_pos = snp_it->first;
                const size_t seq_pos = q + (size_t)((int64_t)genome_pos - r);
                if (seq_pos < rec.seq.size()) {
                    const Genotype readbase = (Genotype)rec.seq[seq_pos];
                    const auto& alleles = pos_allele_map.at(genome_pos);
                    for (size_t i = 0; i < alleles.size(); ++i)
                        if (readbase == alleles[i]) {
                            const SnpPosition snp_pos = snp_it->second;
                            frag.seq_dict[snp_pos] = (Genotype)i;                  // (a later alignment position of the same SNP overwrites, as insert does)
                            frag.qual_dict[snp_pos] = seq_pos < rec.qual.size() ? rec.qual[seq_pos] : 255;
                            if (snp_pos < frag.first_position) frag.first_position = snp_pos;
                            if (snp_pos > frag.last_position) frag.last_position = snp_pos;
                            frag.snp_pos_to_seq_pos[snp_pos] = {0, seq_pos + leading_hardclips};
                            break;
                        }
                }
                ++snp_it;
            }
        }
        if (consumes_q(op)) q += len;
        if (consumes_r(op)) r += len;                                          // D / N over a SNP: pair[0] is None -> no call
    }
    frag_sequences(frag, rec, keep_sequences);
    return frag;
}

void frag_sequences(Frag& frag, const BamRecord& rec, bool keep_sequences) {
    frag.seq_len[0] = rec.seq.size();
    if (keep_sequences) {                                                      // :728-734
        frag.seq_string[0].resize(rec.seq.size());
        for (size_t i = 0; i < rec.seq.size(); ++i) {
            const char c = rec.seq[i];
            frag.seq_string[0][i] = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : ((c == 'a' || c == 'c' || c == 'g' || c == 't') ? (char)(c - 32) : 'A');
        }
        frag.qual_string[0].resize(rec.qual.size());
        for (size_t i = 0; i < rec.qual.size(); ++i) frag.qual_string[0][i] = rec.qual[i] > 222 ? 255 : (uint8_t)(rec.qual[i] + 33);     // checked_add(33).unwrap_or(255)
    }
}

// the same from the two byte ranges floria_hip_blob_sequences returns for a record (bases already A / C / G / T, qualities already + 33): mate 0 or 1 of the fragment
void frag_sequences(Frag& frag, int mate, const uint8_t* bases, const uint8_t* quals, size_t n) {
    frag.seq_string[mate].assign((const char*)bases, n);
    frag.qual_string[mate].assign(quals, quals + n);
}

struct Tagged { uint16_t flags; Frag frag; uint32_t rec_ix = 0; };

// global alignment score of two byte strings, affine gaps: a gap of length n costs open + (n - 1) * extend
int nw_affine_score(const unsigned char* q, int nq, const unsigned char* r, int nr) {
    constexpr int MATCH = 1, MISMATCH = -1, OPEN = -2, EXTEND = -1, NEG = -(1 << 28);
    static thread_local std::vector<int> Mv, Iv, Dv;             // (M: ends in a pair, I: gap in r, D: gap in q), rolling rows
    Mv.assign(nr + 1, NEG); Iv.assign(nr + 1, NEG); Dv.assign(nr + 1, NEG);
    Mv[0] = 0;
    for (int j = 1; j <= nr; ++j) Dv[j] = OPEN + (j - 1) * EXTEND;
    for (int i = 1; i <= nq; ++i) {
        int m_diag = Mv[0], i_diag = Iv[0], d_diag = Dv[0];
        Mv[0] = NEG; Dv[0] = NEG; Iv[0] = OPEN + (i - 1) * EXTEND;
        for (int j = 1; j <= nr; ++j) {
            const int m_up = Mv[j], i_up = Iv[j], d_up = Dv[j];
            const int best_diag = std::max(m_diag, std::max(i_diag, d_diag));
            const auto up = [](unsigned char c) { return (unsigned char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
            const int sub = up(q[i - 1]) == up(r[j - 1]) ? MATCH : MISMATCH;
            const int m_new = best_diag + sub;
            const int i_new = std::max(std::max(m_up, d_up) + OPEN, i_up + EXTEND);               // consume q[i-1] against a gap
            const int d_new = std::max(std::max(Mv[j - 1], Iv[j - 1]) + OPEN, Dv[j - 1] + EXTEND);   // consume r[j-1] against a gap
            m_diag = m_up; i_diag = i_up; d_diag = d_up;
            Mv[j] = m_new; Iv[j] = i_new; Dv[j] = d_new;
        }
    }
    return std::max(Mv[nr], std::max(Iv[nr], Dv[nr]));
}

}  // namespace

// One member of the fixed-block walk family, as scripts/probes/block_walk.c defines it (walk_score): the same cells as nw_affine_score (D best, C gap in the
// column, H gap in the row), but only those a block of B x B cells (plus its border row / column) visits on its way from the top-left corner to cell (nq, nr),
// shifted right or down by `step` cells at a time; a cell whose neighbour was never computed sees -infinity from it.  Never above the exact score.
int walk_affine_score(const unsigned char* q, int nq, const unsigned char* r, int nr, const floria_realign_walk& walk) {
    constexpr int MATCH = 1, MISMATCH = -1, OPEN = -2, EXTEND = -1, NEG = -1000000;
    const int B = (int)walk.block, step = (int)walk.step, W = nr + 1;
    static thread_local std::vector<int> D, C, H;
    static thread_local std::vector<unsigned char> done;
    const size_t cells = (size_t)(nq + 1) * W;
    D.assign(cells, NEG); C.assign(cells, NEG); H.assign(cells, NEG); done.assign(cells, 0);
    const auto up = [](unsigned char c) { return (unsigned char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
    const auto cell = [&](int i, int j) {
        const size_t x = (size_t)i * W + j;
        if (done[x]) return;
        int d = NEG, c = NEG, h = NEG;
        if (i == 0 && j == 0) d = 0;
        else {
            if (i > 0 && done[x - W]) c = std::max(D[x - W] + OPEN, C[x - W] + EXTEND);
            if (j > 0 && done[x - 1]) h = std::max(D[x - 1] + OPEN, H[x - 1] + EXTEND);
            if (i > 0 && j > 0 && done[x - W - 1]) d = D[x - W - 1] + (up(q[i - 1]) == up(r[j - 1]) ? MATCH : MISMATCH);
            d = std::max(d, std::max(c, h));
        }
        D[x] = d < NEG / 2 ? NEG : d; C[x] = c < NEG / 2 ? NEG : c; H[x] = h < NEG / 2 ? NEG : h; done[x] = 1;
    };
    const auto block = [&](int i0, int j0) { for (int i = i0; i <= std::min(i0 + B, nq); ++i) for (int j = j0; j <= std::min(j0 + B, nr); ++j) cell(i, j); };
    int i0 = 0, j0 = 0;
    block(0, 0);
    for (;;) {
        const int ie = std::min(i0 + B, nq), je = std::min(j0 + B, nr);
        if (ie == nq && je == nr) break;
        bool down;
        if (je == nr) down = true;
        else if (ie == nq) down = false;
        else {
            long a = walk.rule ? 0 : NEG, b = a;                      // right border column, bottom border row
            for (int i = i0; i <= ie; ++i) { const size_t x = (size_t)i * W + je; const int v = done[x] ? D[x] : NEG; a = walk.rule ? a + v : std::max<long>(a, v); }
            for (int j = j0; j <= je; ++j) { const size_t x = (size_t)ie * W + j; const int v = done[x] ? D[x] : NEG; b = walk.rule ? b + v : std::max<long>(b, v); }
            down = b > a ? true : (a > b ? false : walk.tie != 0);
        }
        if (down) { i0 += step; if (i0 + B > nq) i0 = std::max(nq - B, 0); }
        else      { j0 += step; if (j0 + B > nr) j0 = std::max(nr - B, 0); }
        block(i0, j0);
    }
    return D[(size_t)nq * W + nr];
}

void parse_realign_spec(const std::string& spec, Options& o) {
    const std::string grammar = "--realign takes exact | block:STEP,RULE,TIE with STEP 1 | 2 | 4 | 8, RULE max | sum, TIE right | down (e.g. block:8,max,right), not '" + spec + "'";
    if (spec == "exact") { o.realign_walk = false; return; }
    if (spec.compare(0, 6, "block:") != 0) throw Error(FLORIA_E_INVALID, grammar);
    std::vector<std::string> f(1);
    for (size_t i = 6; i < spec.size(); ++i) { if (spec[i] == ',') f.emplace_back(); else f.back().push_back(spec[i]); }
    if (f.size() != 3 || (f[0] != "1" && f[0] != "2" && f[0] != "4" && f[0] != "8") || (f[1] != "max" && f[1] != "sum") || (f[2] != "right" && f[2] != "down"))
        throw Error(FLORIA_E_INVALID, grammar);
    o.realign_walk = true;
    o.walk = {8, (uint32_t)(f[0][0] - '0'), f[1] == "sum" ? 1u : 0u, f[2] == "down" ? 1u : 0u};
}

std::string realign_spec(const Options& o) {
    if (!o.realign_walk) return "exact";
    return "block:" + std::to_string(o.walk.step) + (o.walk.rule ? ",sum" : ",max") + (o.walk.tie ? ",down" : ",right");
}

namespace {
// alignment::realign (alignment.rs:7-64)
// `walk`: score with that member of the fixed-block walk family instead of the exact DP (null: exact)
// `queue`: calls the exact shortcut cannot decide are not scored here but appended to the queue (windows + where the result goes) for
// floria_hip_realign, the same DP on the device; null = score them on the host (--ingest-only, tests)
void realign(const std::string& ref_gn, Frag& frag, const BamSeqView& read_seq, const std::map<SnpPosition, GnPosition>& var_to_gn_pos,
             const std::map<GnPosition, std::vector<Genotype>>& gn_pos_to_allele, RealignQueue* queue, const floria_realign_walk* walk) {
    constexpr size_t flank = 16;
    for (auto& kv : frag.seq_dict) {
        const size_t snp_gn_pos = var_to_gn_pos.at(kv.first);
        const size_t snp_q_pos = frag.snp_pos_to_seq_pos.at(kv.first).second;
        if (flank > snp_gn_pos || flank + snp_gn_pos >= ref_gn.size() || flank > snp_q_pos || flank + snp_q_pos >= read_seq.size()) continue;
        unsigned char q[2 * flank], r[2 * flank];
        for (size_t i = 0; i < 2 * flank; ++i) {
            const char c = read_seq[snp_q_pos - flank + i];                      // DnaString::from_acgt_bytes: anything but ACGT becomes A
            q[i] = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (unsigned char)c : ((c == 'a' || c == 'c' || c == 'g' || c == 't') ? (unsigned char)(c - 32) : 'A');
            r[i] = (unsigned char)ref_gn[snp_gn_pos - flank + i];
        }
        const auto& alleles = gn_pos_to_allele.at(snp_gn_pos);
        // Exact shortcut.  Both windows have 2 * flank = 32 bytes, so an alignment with gaps has g >= 1 gap columns on EACH side and
        // scores at most (32 - g) + 2 * (OPEN + (g - 1) * EXTEND) = 30 - 3g <= 27.  With h mismatches outside the SNP column the
        // ungapped alignment scores 32 - 2h for an allele equal to the read's base and 30 - 2h for any other.  So for h <= 2 the
        // first allele equal to the read's base wins strictly (28 > 27); with no such allele and h <= 1 every allele scores
        // 30 - 2h >= 28 and the first one is kept (`score > best_score`).  Everything else takes the DP.
        // Under a fixed-block walk the shortcut stays: a walk's score is never above the exact one (it maximises over fewer paths), and on a window with
        // h <= 2 every member's block keeps the main diagonal, so the ungapped alignment's score is found
        // (tests/test_realign_walk_cpu.py::test_shortcut_is_exact_under_every_walk: all 16 members, both sides of the bound).
        {
            const auto up = [](unsigned char c) { return (unsigned char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
            int h = 0;
            for (size_t i = 0; i < 2 * flank && h <= 2; ++i) h += (i != flank && q[i] != up(r[i]));
            if (h <= 2) {
                size_t a = 0;
                while (a < alleles.size() && up(alleles[a]) != q[flank]) ++a;
                if (a < alleles.size()) { kv.second = (Genotype)a; continue; }
                if (h <= 1) { kv.second = 0; continue; }
            }
        }
        if (queue && alleles.size() <= FLORIA_MAX_ALLELES) {
            const auto up = [](unsigned char c) { return (unsigned char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
            for (size_t i = 0; i < 2 * flank; ++i) { queue->read_windows.push_back(q[i]); queue->ref_windows.push_back(up(r[i])); }
            for (size_t a = 0; a < FLORIA_MAX_ALLELES; ++a) queue->alleles.push_back(a < alleles.size() ? up(alleles[a]) : 0);
            queue->n_alleles.push_back((uint8_t)alleles.size());
            // (the entry lives in the FlatMap's heap storage: it stays where it is when the Frag or the vector holding it MOVES — Frag is nothrow-movable,
            // asserted below — and nothing is inserted into seq_dict between here and realign_queue_on_device; copying a Frag would invalidate it)
            queue->dst.push_back(&kv.second);
            continue;
        }
        int best_score = INT32_MIN;
        Genotype best_geno = 0;
        for (size_t a = 0; a < alleles.size(); ++a) {
            r[flank] = alleles[a];
            const int score = walk ? walk_affine_score(q, 2 * flank, r, 2 * flank, *walk) : nw_affine_score(q, 2 * flank, r, 2 * flank);
            if (score > best_score) { best_score = score; best_geno = (Genotype)a; }
        }
        kv.second = best_geno;
    }
}

// the CG:B,I array among the tags raw[o, end) of a record: -> the offset of its first word and its count; false: there is none (the placeholder CIGAR stays)
bool find_cg_tag(const unsigned char* raw, size_t o, size_t end, const std::string& what, size_t& cg_off, uint32_t& cg_cnt) {
    Cursor d{raw, end, o, what};
    while (d.o + 3 <= end) {
        const unsigned char t0c = raw[d.o], t1c = raw[d.o + 1], ty = raw[d.o + 2];
        d.o += 3;
        size_t len = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
        else if (ty == 's' || ty == 'S') len = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
        else if (ty == 'Z' || ty == 'H') { while (d.o + len < end && raw[d.o + len]) ++len; ++len; }
        else if (ty == 'B') {
            d.need(5);
            const unsigned char sub = raw[d.o];
            uint32_t cnt; memcpy(&cnt, raw + d.o + 1, 4);
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (t0c == 'C' && t1c == 'G' && sub == 'I') { d.o += 5; d.need((size_t)4 * cnt); cg_off = d.o; cg_cnt = cnt; return true; }
            len = 5 + es * cnt;
        } else break;                                                    // unknown type: stop looking
        if (d.o + len > end) break;
        d.o += len;
    }
    return false;
}

// the records of bam.raw[begin, end) (whole records) -> bam.records (views into bam.raw) and bam.by_tid
void decode_records(BamFile& bam, size_t begin, size_t end, const std::string& path, size_t threads) {
    // record boundaries first (a walk over the block_size fields), then the records are decoded independently
    const std::vector<unsigned char>& raw = bam.raw;
    Cursor c{raw.data(), end, begin, path};
    std::vector<size_t> rec_off;
    while (c.o < end) {
        const uint32_t block_size = c.u32(); c.need(block_size);
        rec_off.push_back(c.o);
        c.o += block_size;
    }
    rec_off.push_back(end + 4);
    bam.records.resize(rec_off.size() - 1);
    const size_t per = 256;
    parallel_tasks((bam.records.size() + per - 1) / per, threads, [&](size_t t) {
        for (size_t i = t * per; i < std::min(bam.records.size(), (t + 1) * per); ++i) {
            Cursor d{raw.data(), rec_off[i + 1] - 4, rec_off[i], path};             // (bounded by the record's own end)
            BamRecord& r = bam.records[i];
            r.tid = d.i32(); r.pos = d.i32();
            const uint8_t l_read_name = d.u8(); r.mapq = d.u8(); (void)d.u16();
            const uint16_t n_cigar = d.u16(); r.flags = d.u16();
            const uint32_t l_seq = d.u32(); (void)d.i32(); (void)d.i32(); (void)d.i32();
            d.need(l_read_name); r.qname = std::string_view((const char*)raw.data() + d.o, l_read_name ? l_read_name - 1 : 0); d.o += l_read_name;
            d.need((size_t)4 * n_cigar); r.cigar = BamCigarView{raw.data() + d.o, n_cigar}; d.o += (size_t)4 * n_cigar;
            d.need((size_t)(l_seq + 1) / 2 + l_seq);
            r.seq = BamSeqView{raw.data() + d.o, l_seq}; d.o += (l_seq + 1) / 2;
            r.qual = BamBytesView{raw.data() + d.o, l_seq}; d.o += l_seq;
            // An alignment with more than 65 535 CIGAR operations keeps its real CIGAR in the CG:B,I tag and a placeholder `<l_seq>S<ref_len>N` in the
            // CIGAR field (SAM spec 4.2.2); htslib's bam_read1 puts the real one back (bam_tag2cigar), so the reference sees it.  The other tags are skipped.
            if (n_cigar == 2 && (r.cigar[0] & 15u) == 4u && (r.cigar[0] >> 4) == l_seq && (r.cigar[1] & 15u) == 3u) {
                size_t cg; uint32_t cnt;
                if (find_cg_tag(raw.data(), d.o, rec_off[i + 1] - 4, path, cg, cnt)) r.cigar = BamCigarView{raw.data() + cg, cnt};
            }
        }
    });
    for (size_t i = 0; i < bam.records.size(); ++i) {
        const int32_t tid = bam.records[i].tid;
        if (tid >= 0 && (size_t)tid < bam.by_tid.size()) bam.by_tid[tid].push_back((uint32_t)i);
    }
}

}  // namespace

BamFile read_bam(const std::string& path, size_t threads) {
    const bool trace = getenv("FLORIA_HOST_TRACE") != nullptr;
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    const std::vector<unsigned char> packed = slurp(path);
    if (trace) fprintf(stderr, "[read_bam] file %.3fs (%zu MiB)\n", now() - t0, packed.size() >> 20);
    t0 = now();
    BamFile bam;
    bam.raw = bgzf_inflate_all(packed, path, threads);
    const std::vector<unsigned char>& raw = bam.raw;
    if (trace) fprintf(stderr, "[read_bam] inflate %.3fs (%zu MiB)\n", now() - t0, raw.size() >> 20);
    t0 = now();
    Cursor c{raw.data(), raw.size(), 0, path};
    c.need(4);
    if (memcmp(raw.data(), "BAM\1", 4) != 0) throw Error(FLORIA_E_INVALID, path + " is not a BAM file");
    c.o = 4;
    const uint32_t l_text = c.u32(); c.need(l_text); c.o += l_text;
    const uint32_t n_ref = c.u32();
    for (uint32_t i = 0; i < n_ref; ++i) {
        const uint32_t l_name = c.u32(); c.need(l_name);
        bam.target_names.emplace_back((const char*)raw.data() + c.o, l_name ? l_name - 1 : 0); c.o += l_name;
        bam.target_len.push_back(c.u32());
    }
    bam.by_tid.resize(bam.target_names.size());
    decode_records(bam, c.o, raw.size(), path, threads);
    if (trace) fprintf(stderr, "[read_bam] records %.3fs\n", now() - t0);
    return bam;
}

static_assert(std::is_nothrow_move_constructible<Frag>::value && std::is_nothrow_move_assignable<Frag>::value,
              "RealignQueue::dst points into Frag::seq_dict: a vector of Frags must MOVE its elements when it grows");

// ---- the .bai index ----------------------------------------------------------------------------------------------------------------------
std::string find_bai(const std::string& bam_path) {
    struct stat st;
    const std::string a = bam_path + ".bai";
    if (stat(a.c_str(), &st) == 0 && S_ISREG(st.st_mode)) return a;
    const size_t dot = bam_path.rfind('.');
    if (dot != std::string::npos && bam_path.find('/', dot) == std::string::npos) {
        const std::string b = bam_path.substr(0, dot) + ".bai";
        if (stat(b.c_str(), &st) == 0 && S_ISREG(st.st_mode)) return b;
    }
    return "";
}

BaiIndex read_bai(const std::string& path) {
    const std::vector<unsigned char> raw = slurp(path);
    const auto bad = [&](const std::string& why) { return Error(FLORIA_E_INVALID, path + " is not a valid BAI index: " + why); };
    if (raw.size() < 8) throw Error(FLORIA_E_INVALID, path + " is truncated");
    if (memcmp(raw.data(), "BAI\1", 4) != 0) throw bad("it does not begin with the magic BAI\\1 (a CSI index is not read)");
    Cursor c{raw.data(), raw.size(), 4, path};
    BaiIndex ix;
    ix.path = path;
    const uint32_t n_ref = c.u32();
    c.need((size_t)n_ref * 8);                                  // (n_bin and n_intv of every reference at the least: bounds the allocation below)
    ix.targets.resize(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r) {
        BaiIndex::Target& t = ix.targets[r];
        bool have_meta = false;
        uint64_t meta_beg = 0, meta_end = 0;
        const uint32_t n_bin = c.u32();
        for (uint32_t b = 0; b < n_bin; ++b) {
            const uint32_t bin = c.u32(), n_chunk = c.u32();
            c.need((size_t)n_chunk * 16);
            if (bin == 37450) {                                 // the metadata pseudo-bin: (ref_beg, ref_end), (n_mapped, n_unmapped)
                if (n_chunk != 2) throw bad("the pseudo-bin 37450 of reference " + std::to_string(r) + " has " + std::to_string(n_chunk) + " chunks, not 2");
                meta_beg = c.u64(); meta_end = c.u64(); (void)c.u64(); (void)c.u64();
                have_meta = true;
                continue;
            }
            if (bin > 37448) throw bad("bin " + std::to_string(bin) + " of reference " + std::to_string(r));
            for (uint32_t k = 0; k < n_chunk; ++k) {
                const uint64_t beg = c.u64(), end = c.u64();
                if (!t.has_records || beg < t.begin) t.begin = beg;
                if (!t.has_records || end > t.end) t.end = end;
                t.has_records = true;
            }
        }
        if (have_meta && t.has_records && meta_beg != t.begin)
            throw bad("reference " + std::to_string(r) + ": ref_beg of the pseudo-bin is not the smallest chunk begin of its bins");
        if (have_meta && t.has_records) t.end = std::max(t.end, meta_end);
        const uint32_t n_intv = c.u32();
        c.need((size_t)n_intv * 8);
        c.o += (size_t)n_intv * 8;
    }
    if (c.o + 8 == raw.size()) { ix.n_no_coor = c.u64(); ix.has_n_no_coor = true; }
    else if (c.o != raw.size()) throw bad(std::to_string(raw.size() - c.o) + " bytes follow the last reference");
    return ix;
}

// ---- BamStream -------------------------------------------------------------------------------------------------------------------------
struct BamStream::Impl {
    std::string path;
    size_t threads = 1;
    int fd = -1;
    const unsigned char* map = nullptr;
    size_t map_len = 0;
    // BGZF members from the start of the file (empty: not a BGZF file -> `whole`).  Without an index all of them, walked at open; with one, those walked
    // so far (have_block walks on): the stretches select() asks for keep member lists of their own, from each seek point on
    std::vector<BgzfBlock> blocks;
    size_t walked = 0;                        // file offset behind the last member of `blocks`
    bool bgzf = false;
    // the index and the selection
    bool indexed = false;
    BaiIndex bai;
    std::vector<int32_t> sel;                 // select(): ascending
    bool selecting = false, sel_done = false;
    size_t sel_pos = 0;
    size_t members_inflated = 0;              // since select()
    struct CachedMember { size_t in_off = SIZE_MAX; std::vector<unsigned char> bytes; };
    CachedMember cache[2];                    // the last two members of the previous stretch: the next selected target often begins in them

    bool have_block(size_t i) {               // is there a member i?  (walks the headers up to it)
        while (i >= blocks.size() && walked < map_len) {
            size_t bsize; uint32_t isize;
            if (!bgzf_member(ByteSpan{map, map_len}, walked, bsize, isize)) throw Error(FLORIA_E_INVALID, path + " is not a valid BGZF/gzip file");
            blocks.push_back({walked, bsize, blocks.empty() ? 0 : blocks.back().out_off + blocks.back().out_len, isize});
            walked += bsize;
        }
        return i < blocks.size();
    }
    BamFile whole;                            // fallback: the file read at once
    bool whole_given = false;
    std::vector<std::string> names;
    std::vector<uint64_t> lens;
    size_t first_block = 0, first_skip = 0;   // where the records begin: member index and offset inside its inflated bytes
    // position
    size_t bi = 0;                            // next member to inflate
    std::vector<unsigned char> carry;         // inflated bytes not handed out yet (starts at a record boundary)
    int32_t done_upto = 0;                    // targets < done_upto have been handed out
    int32_t last_tid_seen = 0;
    bool eof = false;
    size_t peak = 0;

    void inflate_range(size_t b0, size_t b1, unsigned char* dst) const { inflate_range(blocks, b0, b1, dst); }
    void inflate_run(const std::vector<BgzfBlock>& blocks, size_t b0, size_t b1, unsigned char* dst) const {            // members [b0, b1) -> dst (contiguous), on this thread
        const size_t base = blocks[b0].out_off;
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) throw Error(FLORIA_E_NOMEM, "inflateInit2 failed");
        for (size_t b = b0; b < b1; ++b) {
            const BgzfBlock& k = blocks[b];
            zs.next_in = const_cast<unsigned char*>(map) + k.in_off; zs.avail_in = (uInt)k.in_len;
            unsigned char dummy;
            zs.next_out = k.out_len ? dst + (k.out_off - base) : &dummy; zs.avail_out = (uInt)k.out_len;
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.avail_out != 0) { inflateEnd(&zs); throw Error(FLORIA_E_INVALID, path + " is not a valid BGZF/gzip file"); }
            inflateReset(&zs);
        }
        inflateEnd(&zs);
    }
    void inflate_range(const std::vector<BgzfBlock>& blocks, size_t b0, size_t b1, unsigned char* dst) const {          // the same on the threads
        const size_t per = 32;
        parallel_tasks((b1 - b0 + per - 1) / per, threads, [&](size_t t) {
            const size_t k0 = b0 + t * per, k1 = std::min(b1, b0 + (t + 1) * per);
            inflate_run(blocks, k0, k1, dst + (blocks[k0].out_off - blocks[b0].out_off));
        });
    }

    // ---- reading through the index.  A stretch is what the file holds of one selected target: from the virtual offset the index gives for its first record
    // up to the first record of another target, the unplaced tail or the end of the file.  The index's end offset says which members to inflate (all stretches
    // of a segment side by side, into one buffer); where a stretch really ends is read from its records, with members of look-ahead where the index's end is
    // the end of a member or short of the truth.
    struct Stretch {
        int32_t tid = 0;
        size_t u0 = 0;                          // the first record's offset inside the first member
        std::vector<BgzfBlock> bl;              // the members from the first one on, out_off counted from its first inflated byte
        size_t n_hint = 0, at = 0;              // bl[0, n_hint) are in the region; `at`: file offset behind bl.back()
        size_t roff = 0, rlen = 0;              // the region: inflated bytes of bl[0, n_hint) in the segment's buffer
        size_t lead = 0;                        // leading members the stretch before it (or the cache) already holds: copied, not inflated
        size_t rec_end = 0;                     // buffer offset behind the last whole record of tid inside the region
        std::vector<unsigned char> tail;        // the region's bytes from rec_end on and the look-ahead members behind them
        size_t tail_recs = 0;                   // bytes of whole records of tid at the front of `tail`
    };
    Error bad_index(int32_t t, const std::string& why) const {
        return Error(FLORIA_E_INVALID, bai.path + ": " + why + " (target " + names[(size_t)t] + " of " + path + "); rebuild the index, or run with --no-index");
    }
    bool stretch_more(Stretch& s) const {         // the header of one more member; false at the end of the file
        if (s.at >= map_len) return false;
        size_t bsize; uint32_t isize;
        if (!bgzf_member(ByteSpan{map, map_len}, s.at, bsize, isize)) {
            if (s.bl.empty()) throw bad_index(s.tid, "the offset of the first record does not land on the start of a BGZF member");
            throw Error(FLORIA_E_INVALID, path + " is not a valid BGZF/gzip file");
        }
        s.bl.push_back({s.at, bsize, s.bl.empty() ? 0 : s.bl.back().out_off + s.bl.back().out_len, isize});
        s.at += bsize;
        return true;
    }
    Stretch plan_stretch(int32_t t) const {
        const BaiIndex::Target& T = bai.targets[(size_t)t];
        const size_t c0 = (size_t)(T.begin >> 16), ce = (size_t)(T.end >> 16), ue = (size_t)(T.end & 0xffff);
        if (c0 >= map_len) throw bad_index(t, "the offset of the first record lies beyond the file");
        Stretch s;
        s.tid = t; s.u0 = (size_t)(T.begin & 0xffff); s.at = c0;
        stretch_more(s);
        if (s.u0 > s.bl[0].out_len) throw bad_index(t, "the offset of the first record lies beyond its BGZF member");
        if (ce <= map_len) while (s.at < map_len && (s.at < ce || (s.at == ce && ue > 0))) stretch_more(s);      // (an end beyond the file is no hint)
        s.n_hint = s.bl.size();
        s.rlen = s.bl.back().out_off + s.bl.back().out_len;
        return s;
    }
    // whole records of `tid` in [p + o, p + n): o moves behind them; true: a record of another target (or an unplaced one) follows, the stretch is complete
    bool scan_stretch(const Stretch& s, const unsigned char* p, size_t n, size_t& o, bool& first) const {
        while (o + 8 <= n) {
            uint32_t bs; memcpy(&bs, p + o, 4);
            int32_t tid; memcpy(&tid, p + o + 4, 4);
            if (tid != s.tid) { if (first) throw bad_index(s.tid, "the record at the offset of the first record belongs to another target"); return true; }
            if (bs < 32) throw Error(FLORIA_E_INVALID, path + ": malformed BAM record");
            if (o + 4 + (size_t)bs > n) break;
            first = false;
            o += 4 + (size_t)bs;
        }
        return false;
    }
    // member k of a stretch's list where a neighbour already holds its bytes: in the region of `other` (buf) or in the cache; null: it has to be inflated
    const unsigned char* held(const BgzfBlock& m, const Stretch* other, const unsigned char* buf) const {
        if (other) for (size_t k = 0; k < other->n_hint; ++k) {
            if (other->bl[k].in_off > m.in_off) break;
            if (other->bl[k].in_off == m.in_off && other->bl[k].out_len == m.out_len) return buf + other->roff + other->bl[k].out_off;
        }
        for (const CachedMember& c : cache) if (c.in_off == m.in_off && c.bytes.size() == m.out_len) return c.bytes.empty() ? buf : c.bytes.data();
        return nullptr;
    }
    // The records of the planned stretches -> buf, target after target
    void read_stretches(std::vector<Stretch>& S, std::vector<unsigned char>& buf) {
        size_t total = 0;
        for (Stretch& s : S) { s.roff = total; total += s.rlen; }
        buf.resize(total);
        // one pass over every member of every stretch on the threads, but for the leading members that the stretch before holds as its last ones (a target
        // begins in the member the one before it ends in) or that the cache holds from the segment before
        struct Job { size_t s, k0, k1; };
        std::vector<Job> jobs;
        const size_t per = 8;
        for (size_t i = 0; i < S.size(); ++i) {
            Stretch& s = S[i];
            const Stretch* before = i ? &S[i - 1] : nullptr;
            while (s.lead < s.n_hint && held(s.bl[s.lead], before, buf.data())) ++s.lead;
            for (size_t k = s.lead; k < s.n_hint; k += per) jobs.push_back({i, k, std::min(s.n_hint, k + per)});
            members_inflated += s.n_hint - s.lead;
        }
        parallel_tasks(jobs.size(), threads, [&](size_t j) {
            const Stretch& s = S[jobs[j].s];
            inflate_run(s.bl, jobs[j].k0, jobs[j].k1, buf.data() + s.roff + s.bl[jobs[j].k0].out_off);
        });
        for (size_t i = 0; i < S.size(); ++i)                                       // (ascending: the stretch before is whole when its bytes are taken)
            for (size_t k = 0; k < S[i].lead; ++k) {
                const BgzfBlock& m = S[i].bl[k];
                if (m.out_len) memcpy(buf.data() + S[i].roff + m.out_off, held(m, i ? &S[i - 1] : nullptr, buf.data()), m.out_len);
            }
        peak = std::max(peak, buf.size());
        // where every stretch ends
        bool any_tail_records = false;
        for (size_t i = 0; i < S.size(); ++i) {
            Stretch& s = S[i];
            size_t o = s.u0;
            bool first = true;
            bool ended = scan_stretch(s, buf.data() + s.roff, s.rlen, o, first);
            s.rec_end = s.roff + o;
            if (ended) continue;
            // the region ends with the stretch's last record, or inside a record: look ahead, first in what the next stretch or the cache holds
            s.tail.assign(buf.begin() + (ptrdiff_t)s.rec_end, buf.begin() + (ptrdiff_t)(s.roff + s.rlen));
            size_t p = 0, look = 1;
            while (!ended) {
                const size_t had = s.bl.size();
                for (size_t k = 0; k < look && stretch_more(s); ++k) {}
                if (s.bl.size() == had) {
                    if (p != s.tail.size()) throw Error(FLORIA_E_INVALID, path + " is truncated");
                    if (first) throw bad_index(s.tid, "there is no record at the offset of the first record");
                    break;
                }
                look *= 2;
                for (size_t k = had; k < s.bl.size(); ++k) {
                    const BgzfBlock& m = s.bl[k];
                    const size_t at = s.tail.size();
                    s.tail.resize(at + m.out_len);
                    const unsigned char* src = held(m, i + 1 < S.size() ? &S[i + 1] : nullptr, buf.data());
                    if (src) { if (m.out_len) memcpy(s.tail.data() + at, src, m.out_len); }
                    else { inflate_run(s.bl, k, k + 1, s.tail.data() + at); ++members_inflated; }
                }
                ended = scan_stretch(s, s.tail.data(), s.tail.size(), p, first);
            }
            s.tail_recs = p;
            any_tail_records |= p != 0;
        }
        // the last two members of the last stretch stay at hand: the first target of the next segment often begins in them
        if (!S.empty()) {
            const Stretch& s = S.back();
            CachedMember keep[2];
            for (size_t j = 0; j < 2 && j < s.bl.size(); ++j) {
                const size_t k = s.bl.size() - 1 - j;
                const BgzfBlock& m = s.bl[k];
                const unsigned char* src = k < s.n_hint ? buf.data() + s.roff + m.out_off
                                                        : s.tail.data() + (s.roff + s.rlen - s.rec_end) + (m.out_off - s.bl[s.n_hint].out_off);
                keep[j].in_off = m.in_off;
                keep[j].bytes.assign(src, src + m.out_len);
            }
            for (size_t j = 0; j < 2; ++j) cache[j] = std::move(keep[j]);
        }
        // the records of the stretches, one behind the other
        if (!any_tail_records) {
            size_t d = 0;
            for (const Stretch& s : S) { const size_t n = s.rec_end - (s.roff + s.u0); memmove(buf.data() + d, buf.data() + s.roff + s.u0, n); d += n; }
            buf.resize(d);
        } else {                                       // (an index whose end offsets fall short: records came by look-ahead)
            std::vector<unsigned char> out;
            for (const Stretch& s : S) {
                out.insert(out.end(), buf.begin() + (ptrdiff_t)(s.roff + s.u0), buf.begin() + (ptrdiff_t)s.rec_end);
                out.insert(out.end(), s.tail.begin(), s.tail.begin() + (ptrdiff_t)s.tail_recs);
            }
            peak = std::max(peak, buf.size() + out.size());
            buf.swap(out);
        }
    }

    // ---- --inflate device (BamStream::inflate_on_device): the same segments planned from member headers, inflated and read on the device
    floria_hip_ctx* dctx = nullptr;
    BamStream::DeviceUse duse;
    size_t dev_skip = 0;                      // without an index: offset of the next segment's first record inside member `bi`

    // the adjacent members bl[b0, b1) -> a blob, and the table of the chains that begin at `begin` and are open to the blob's end
    std::unique_ptr<DeviceSegment> device_read(const std::vector<BgzfBlock>& bl, size_t b0, size_t b1, const std::vector<uint64_t>& begin, uint32_t flags) {
        const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        std::unique_ptr<DeviceSegment> d(new DeviceSegment);
        d->ctx = dctx;
        std::vector<uint64_t> off(b1 - b0);
        std::vector<uint32_t> len(b1 - b0);
        for (size_t b = b0; b < b1; ++b) { off[b - b0] = bl[b].in_off; len[b - b0] = (uint32_t)bl[b].in_len; }
        double t0 = now();
        if (const int rc = floria_hip_inflate_bgzf(dctx, map, map_len, off.data(), len.data(), (uint32_t)(b1 - b0), &d->blob))
            throw Error(rc, path + ": floria_hip_inflate_bgzf: " + floria_hip_last_error());
        duse.inflate_s += now() - t0;
        duse.members += b1 - b0; members_inflated += b1 - b0;
        duse.compressed_bytes += bl[b1 - 1].in_off + bl[b1 - 1].in_len - bl[b0].in_off;
        const uint64_t blob_bytes = floria_hip_blob_bytes(d->blob);
        duse.inflated_bytes += blob_bytes;
        for (const uint64_t b : begin) if (b > blob_bytes) throw Error(FLORIA_E_INVALID, path + ": a chain of records begins beyond the inflated members");
        const std::vector<uint64_t> end(begin.size(), blob_bytes);
        t0 = now();
        if (const int rc = floria_hip_blob_records_opt(dctx, d->blob, begin.data(), end.data(), (uint32_t)begin.size(), flags, &d->table))
            throw Error(rc, path + ": floria_hip_blob_records_opt: " + floria_hip_last_error());
        duse.table_s += now() - t0;
        return d;
    }
    // records [lo, hi) of the table -> seg.records (places as blob offsets, names as views into the table) and seg.by_tid
    void device_records(BamFile& seg, uint64_t lo, uint64_t hi) {
        DeviceSegment& d = *seg.dev;
        const floria_blob_records& T = *d.table;
        const size_t n = (size_t)(hi - lo);
        seg.records.resize(n); d.rec_off.resize(n); d.rec_end.resize(n);
        const auto place = [](uint64_t o) { return (const unsigned char*)(uintptr_t)o; };
        std::vector<unsigned char> rec;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t j = lo + i, o = T.offset[j];
            const size_t l_name = T.l_read_name[j], n_cigar = T.n_cigar_op[j], l_seq = T.l_seq[j], whole = 4 + (size_t)T.block_size[j];
            const uint64_t cig = o + 36 + l_name, sq = cig + 4 * n_cigar, ql = sq + (l_seq + 1) / 2;
            if (36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq > whole) throw Error(FLORIA_E_INVALID, path + ": malformed BAM record");
            BamRecord& r = seg.records[i];
            r.tid = T.ref_id[j]; r.pos = T.pos[j]; r.mapq = T.mapq[j]; r.flags = T.flag[j];
            r.qname = std::string_view((const char*)T.names + T.name_off[j], l_name ? l_name - 1 : 0);
            r.cigar = BamCigarView{place(cig), n_cigar}; r.seq = BamSeqView{place(sq), l_seq}; r.qual = BamBytesView{place(ql), l_seq};
            d.rec_off[i] = o; d.rec_end[i] = o + whole;
            // the kSmN placeholder of a CG-tag record (decode_records): its bytes come down, the tag scan finds the real CIGAR, whose place in the blob goes into the view
            if (n_cigar == 2 && T.cigar0[j] == ((uint32_t)l_seq << 4 | 4u)) {
                rec.resize(whole);
                if (const int rc = floria_hip_blob_download(d.blob, o, rec.data(), whole)) throw Error(rc, path + ": floria_hip_blob_download: " + floria_hip_last_error());
                duse.cg_bytes_down += whole;
                uint32_t c1; memcpy(&c1, rec.data() + (size_t)(cig - o) + 4, 4);
                size_t cg; uint32_t cnt;
                if ((c1 & 15u) == 3u && find_cg_tag(rec.data(), (size_t)(ql - o) + l_seq, whole, path, cg, cnt)) r.cigar = BamCigarView{place(o + cg), cnt};
            }
            if (r.tid >= 0 && (size_t)r.tid < seg.by_tid.size()) seg.by_tid[(size_t)r.tid].push_back((uint32_t)i);
        }
    }
    void device_segment(BamFile& seg, std::unique_ptr<DeviceSegment> d, uint64_t rec_lo, uint64_t rec_hi, int32_t upto) {
        seg = BamFile();
        seg.target_names = names; seg.target_len = lens;
        seg.by_tid.resize(names.size());
        seg.dev = std::move(d);
        if (seg.dev->table) device_records(seg, rec_lo, rec_hi);
        seg.tid_begin = done_upto; seg.tid_end = upto;
        done_upto = upto;
        ++duse.segments;
    }
    // with an index: the selected targets in header order, as many as the window takes and as lie side by side in the file
    bool next_device_indexed(BamFile& seg, size_t min_bytes) {
        if (sel_done) return false;
        const int32_t n_targets = (int32_t)names.size();
        int32_t upto = done_upto;
        bool any = false;
        std::vector<Stretch> st;
        size_t planned = 0, run_end = 0;                                           // run_end: file offset behind the last member the index's ends ask for
        while (sel_pos < sel.size() && (!any || planned < min_bytes)) {
            const int32_t t = sel[sel_pos];
            if (bai.targets[(size_t)t].has_records) {
                Stretch s = plan_stretch(t);
                const size_t c0 = s.bl[0].in_off;
                // everything between the first and the last member goes up: the segment ends where the next target begins neither in the run nor in the member behind it
                if (!st.empty() && (c0 > run_end || c0 < st[0].bl[0].in_off)) break;
                run_end = std::max(run_end, s.at); planned += s.rlen;
                st.push_back(std::move(s));
            }
            ++sel_pos; upto = t + 1; any = true;
        }
        if (sel_pos >= sel.size()) { upto = n_targets; sel_done = true; }
        std::unique_ptr<DeviceSegment> d(new DeviceSegment);
        d->ctx = dctx;
        for (size_t look = 1; !st.empty(); look *= 2) {
            Stretch run;
            run.tid = st[0].tid; run.at = st[0].bl[0].in_off;
            while (run.at < run_end && stretch_more(run)) {}
            for (size_t k = 0; k < look && stretch_more(run); ++k) {}
            const bool at_eof = run.at >= map_len;
            std::vector<uint64_t> begin;
            for (const Stretch& s : st) {
                const auto m = std::lower_bound(run.bl.begin(), run.bl.end(), s.bl[0].in_off, [](const BgzfBlock& b, size_t o) { return b.in_off < o; });
                if (m == run.bl.end() || m->in_off != s.bl[0].in_off) throw bad_index(s.tid, "the offset of the first record does not land on the start of a BGZF member");
                begin.push_back(m->out_off + s.u0);
            }
            d.reset();                                                                // (a re-plan: the blob that fell short goes before the larger one is made)
            d = device_read(run.bl, 0, run.bl.size(), begin, FLORIA_CHAIN_ONE_REF | FLORIA_CHAIN_CUT_TAIL);
            const floria_blob_records& T = *d->table;
            bool short_of_end = false;
            for (size_t c = 0; c < st.size(); ++c) {
                const bool has = T.chain_rec_off[c + 1] > T.chain_rec_off[c];
                if (has && T.ref_id[T.chain_rec_off[c]] != st[c].tid) throw bad_index(st[c].tid, "the record at the offset of the first record belongs to another target");
                if (T.chain_why[c] == 2) { if (!has) throw bad_index(st[c].tid, "the record at the offset of the first record belongs to another target"); continue; }
                if (!at_eof) { short_of_end = true; continue; }                       // the blob ended before another target did: look further ahead
                if (T.chain_stop[c] != floria_hip_blob_bytes(d->blob)) throw Error(FLORIA_E_INVALID, path + " is truncated");
                if (!has) throw bad_index(st[c].tid, "there is no record at the offset of the first record");
            }
            if (!short_of_end) break;
            ++duse.replanned;
        }
        const uint64_t n_records = d->table ? d->table->n_records : 0;
        device_segment(seg, std::move(d), 0, n_records, upto);
        return true;
    }
    // without an index (or with --no-index): members in file order until their ISIZEs sum to the window, one chain
    bool next_device_stream(BamFile& seg, size_t min_bytes) {
        const int32_t n_targets = (int32_t)names.size();
        if (eof && done_upto >= n_targets) return false;
        size_t want = std::max<size_t>(min_bytes, 1 << 16);
        for (;;) {
            size_t b1 = bi;
            uint64_t sum = 0;
            while (have_block(b1) && sum < dev_skip + want) sum += blocks[b1++].out_len;
            const bool at_end = !have_block(b1);
            std::unique_ptr<DeviceSegment> d(new DeviceSegment);
            d->ctx = dctx;
            if (b1 == bi) {                                                            // no member is left: the targets not handed out yet have no record
                if (dev_skip) throw Error(FLORIA_E_INVALID, path + " is truncated");
                eof = true;
                device_segment(seg, std::move(d), 0, 0, n_targets);
                return true;
            }
            d = device_read(blocks, bi, b1, std::vector<uint64_t>{dev_skip}, FLORIA_CHAIN_CUT_TAIL);
            const floria_blob_records& T = *d->table;
            if (at_end && T.chain_why[0] != 0) throw Error(FLORIA_E_INVALID, path + " is truncated");
            // [0, cut) = the records of targets that are certainly complete (the walk of next() on the table's refIDs)
            uint64_t first_of_last = 0;
            int32_t cur_tid = INT32_MIN, prev = last_tid_seen;
            bool saw_unmapped = false;
            for (uint64_t i = 0; i < T.n_records; ++i) {
                const int32_t tid = T.ref_id[i];
                if (tid < 0) { if (!saw_unmapped) { saw_unmapped = true; first_of_last = i; cur_tid = n_targets; } }
                else if (saw_unmapped || tid < prev) throw Error(FLORIA_E_INVALID, path + " is not sorted by reference sequence (floria needs a coordinate-sorted, indexed BAM; so does this reader)");
                else if (tid != cur_tid) { cur_tid = tid; first_of_last = i; prev = tid; }
            }
            const bool closing = at_end || saw_unmapped;
            uint64_t cut; int32_t complete_upto;
            if (closing) { cut = saw_unmapped ? first_of_last : T.n_records; complete_upto = n_targets; }
            else { cut = first_of_last; complete_upto = cur_tid == INT32_MIN ? done_upto : std::min(cur_tid, n_targets); }
            if (!closing && (cut == 0 || complete_upto <= done_upto)) { want = std::max<size_t>(want * 2, (size_t)sum * 2); continue; }      // one target fills the window: read on
            if (closing) eof = true;
            else {
                // the next segment begins at the member that holds the first record of the incomplete target; the members from there on are inflated again
                const uint64_t o = T.offset[cut], base = blocks[bi].out_off;
                size_t m = (size_t)(std::upper_bound(blocks.begin() + (ptrdiff_t)bi, blocks.begin() + (ptrdiff_t)b1, base + o,
                                                     [](uint64_t v, const BgzfBlock& b) { return v < b.out_off; }) - blocks.begin()) - 1;
                duse.carried_members += b1 - m;
                dev_skip = (size_t)(base + o - blocks[m].out_off); bi = m;
            }
            last_tid_seen = std::max(last_tid_seen, std::min(prev, n_targets));
            device_segment(seg, std::move(d), 0, cut, complete_upto);
            return true;
        }
    }
};

BamStream::BamStream(const std::string& path, size_t threads, bool use_index) : p_(new Impl) {
    Impl& I = *p_;
    I.path = path; I.threads = std::max<size_t>(1, threads);
    I.fd = open(path.c_str(), O_RDONLY);
    if (I.fd < 0) throw Error(FLORIA_E_INVALID, "cannot open " + path);
    struct stat st;
    if (fstat(I.fd, &st) != 0 || st.st_size <= 0) throw Error(FLORIA_E_INVALID, path + " is empty or unreadable");
    I.map_len = (size_t)st.st_size;
    void* m = mmap(nullptr, I.map_len, PROT_READ, MAP_PRIVATE, I.fd, 0);
    if (m == MAP_FAILED) throw Error(FLORIA_E_INVALID, "cannot map " + path);
    I.map = (const unsigned char*)m;
    const std::string bai_path = use_index ? find_bai(path) : std::string();
    size_t bsize0; uint32_t isize0;
    if (!bai_path.empty() && bgzf_member(ByteSpan{I.map, I.map_len}, 0, bsize0, isize0)) {
        // with an index the member headers are walked as far as the reading gets, not to the end of the file
        I.bai = read_bai(bai_path);
        I.indexed = I.bgzf = true;
        struct stat sx;
        if (stat(bai_path.c_str(), &sx) == 0 && (sx.st_mtim.tv_sec < st.st_mtim.tv_sec || (sx.st_mtim.tv_sec == st.st_mtim.tv_sec && sx.st_mtim.tv_nsec < st.st_mtim.tv_nsec)))
            fprintf(stderr, "floria-hip: warning: the index %s is older than %s; it is used all the same (rebuild it, or run with --no-index, if the BAM was written again since)\n",
                    bai_path.c_str(), path.c_str());
    } else {
        I.bgzf = bgzf_index(ByteSpan{I.map, I.map_len}, I.blocks) && !I.blocks.empty();
        if (I.bgzf) I.walked = I.map_len;
    }
    if (!I.bgzf) {                                   // plain gzip (or anything else zlib understands): no member index, the file is read whole
        I.whole = read_bam(path, threads);
        I.names = I.whole.target_names; I.lens = I.whole.target_len;
        I.whole.tid_begin = 0; I.whole.tid_end = (int32_t)I.names.size();
        return;
    }
    // the header: inflate members until magic, text and reference list are complete
    std::vector<unsigned char> head;
    size_t b1 = 0;
    auto have = [&](size_t need) {
        while (head.size() < need && I.have_block(b1)) {
            const size_t o = head.size();
            head.resize(o + I.blocks[b1].out_len);
            if (I.blocks[b1].out_len) { std::vector<unsigned char> tmp(I.blocks[b1].out_len); I.inflate_range(b1, b1 + 1, tmp.data()); memcpy(head.data() + o, tmp.data(), tmp.size()); }
            ++b1;
        }
        if (head.size() < need) throw Error(FLORIA_E_INVALID, path + " is truncated");
    };
    have(12);
    if (memcmp(head.data(), "BAM\1", 4) != 0) throw Error(FLORIA_E_INVALID, path + " is not a BAM file");
    uint32_t l_text; memcpy(&l_text, head.data() + 4, 4);
    size_t o = 8 + (size_t)l_text;
    have(o + 4);
    uint32_t n_ref; memcpy(&n_ref, head.data() + o, 4); o += 4;
    for (uint32_t i = 0; i < n_ref; ++i) {
        have(o + 4);
        uint32_t l_name; memcpy(&l_name, head.data() + o, 4); o += 4;
        have(o + l_name + 4);
        I.names.emplace_back((const char*)head.data() + o, l_name ? l_name - 1 : 0); o += l_name;
        uint32_t ln; memcpy(&ln, head.data() + o, 4); o += 4;
        I.lens.push_back(ln);
    }
    // the records start at inflated offset o: find its member
    size_t b = 0;
    while (I.have_block(b) && I.blocks[b].out_off + I.blocks[b].out_len <= o) ++b;
    I.first_block = b; I.first_skip = I.have_block(b) ? o - I.blocks[b].out_off : 0;
    if (I.indexed) {
        if (I.bai.targets.size() != I.names.size())
            throw Error(FLORIA_E_INVALID, I.bai.path + " indexes " + std::to_string(I.bai.targets.size()) + " reference sequences, the header of " + path + " has " +
                                          std::to_string(I.names.size()) + ": it is the index of another file");
        for (size_t t = 0; t < I.bai.targets.size(); ++t)
            if (I.bai.targets[t].has_records && (I.bai.targets[t].begin >> 16) >= I.map_len)
                throw Error(FLORIA_E_INVALID, I.bai.path + ": the offset of the first record of target " + I.names[t] + " lies beyond the end of " + path +
                                              "; rebuild the index, or run with --no-index");
    }
    rewind();
}
BamStream::~BamStream() {
    if (p_->map) munmap(const_cast<unsigned char*>(p_->map), p_->map_len);
    if (p_->fd >= 0) close(p_->fd);
}
const std::vector<std::string>& BamStream::target_names() const { return p_->names; }
size_t BamStream::peak_buffer_bytes() const { return p_->peak; }
const std::string& BamStream::index_path() const { return p_->bai.path; }
void BamStream::select(const std::vector<int32_t>& tids) {
    Impl& I = *p_;
    if (!I.indexed) return;
    I.sel = tids;
    std::sort(I.sel.begin(), I.sel.end());
    I.sel.erase(std::unique(I.sel.begin(), I.sel.end()), I.sel.end());
    if (!I.sel.empty() && (I.sel.front() < 0 || (size_t)I.sel.back() >= I.names.size())) throw Error(FLORIA_E_INVALID, "BamStream::select: no such target");
    I.selecting = true; I.sel_done = false; I.sel_pos = 0; I.done_upto = 0; I.members_inflated = 0;
    I.carry.clear();
    for (Impl::CachedMember& m : I.cache) m = Impl::CachedMember();
}
BamStream::IndexUse BamStream::index_use() const {
    Impl& I = *p_;
    try { I.have_block(SIZE_MAX); } catch (const Error&) {}            // (a member the reading never reached: counted up to it)
    return {I.sel.size(), I.members_inflated, I.blocks.size()};
}
void BamStream::inflate_on_device(floria_hip_ctx* ctx) {
    Impl& I = *p_;
    if (!I.bgzf)
        throw Error(FLORIA_E_UNSUPPORTED, I.path + " is a gzip file without BGZF members: --inflate device inflates member by member and cannot read it; run with --inflate host");
    I.dctx = ctx;
    // the pass begins at the first record again, with nothing inflated on the host: the member the header ends in goes to the device with the others
    I.carry.clear();
    I.bi = I.first_block; I.dev_skip = I.first_skip;
}
BamStream::DeviceUse BamStream::device_use() const { return p_->duse; }
void BamStream::rewind() {
    Impl& I = *p_;
    if (!I.bgzf) { if (I.whole_given) { I.whole = read_bam(I.path, I.threads); I.whole.tid_begin = 0; I.whole.tid_end = (int32_t)I.names.size(); } I.whole_given = false; return; }
    I.bi = I.first_block; I.carry.clear(); I.done_upto = 0; I.last_tid_seen = 0; I.eof = false;
    I.sel_pos = 0; I.sel_done = false;
    if (I.bgzf && I.have_block(I.first_block) && I.first_skip) {       // the rest of the member the header ends in
        std::vector<unsigned char> tmp(I.blocks[I.first_block].out_len);
        I.inflate_range(I.first_block, I.first_block + 1, tmp.data());
        I.carry.assign(tmp.begin() + (ptrdiff_t)I.first_skip, tmp.end());
        I.bi = I.first_block + 1;
    }
}
bool BamStream::next(BamFile& seg, size_t min_bytes) {
    Impl& I = *p_;
    const int32_t n_targets = (int32_t)I.names.size();
    if (!I.bgzf) {
        if (I.whole_given) return false;
        I.whole_given = true;
        seg = std::move(I.whole);             // (a rewind() after this would need the file again: the whole-file fallback is single-pass unless re-read)
        I.whole = BamFile();
        I.peak = std::max(I.peak, seg.raw.size());
        return true;
    }
    if (I.dctx) return I.selecting ? I.next_device_indexed(seg, min_bytes) : I.next_device_stream(seg, min_bytes);
    std::vector<unsigned char> buf;
    if (I.selecting) {
        // the selected targets in header order, each from its indexed offset, as many as the window takes; the targets between them have no records here
        if (I.sel_done) return false;
        int32_t upto = I.done_upto;
        bool any = false;
        std::vector<Impl::Stretch> stretches;
        size_t planned = 0;
        while (I.sel_pos < I.sel.size() && (!any || planned < min_bytes)) {
            const int32_t t = I.sel[I.sel_pos++];
            if (I.bai.targets[(size_t)t].has_records) { stretches.push_back(I.plan_stretch(t)); planned += stretches.back().rlen; }
            upto = t + 1; any = true;
        }
        I.read_stretches(stretches, buf);
        if (I.sel_pos >= I.sel.size()) { upto = n_targets; I.sel_done = true; }
        seg = BamFile();
        seg.target_names = I.names; seg.target_len = I.lens;
        seg.by_tid.resize(I.names.size());
        seg.raw = std::move(buf);
        I.peak = std::max(I.peak, seg.raw.size());
        decode_records(seg, 0, seg.raw.size(), I.path, I.threads);
        seg.tid_begin = I.done_upto; seg.tid_end = upto;
        I.done_upto = upto;
        return true;
    }
    if (I.eof && I.done_upto >= n_targets) return false;
    size_t want = std::max<size_t>(min_bytes, 1 << 16);
    for (;;) {
        // ---- inflate members until the buffer holds `want` bytes (or the file ends)
        size_t b1 = I.bi, add = 0;
        while (I.have_block(b1) && I.carry.size() + buf.size() + add < want) add += I.blocks[b1++].out_len;
        if (buf.empty()) { buf.swap(I.carry); I.carry.clear(); }
        if (b1 > I.bi) {
            const size_t o = buf.size();
            buf.resize(o + add);
            I.inflate_range(I.bi, b1, buf.data() + o);
            I.bi = b1;
        }
        const bool at_end = !I.have_block(I.bi);
        // ---- walk the records: [0, cut) = whole records of targets that are certainly complete
        size_t o = 0, last_start_of_tid = 0, whole_end = 0;
        int32_t cur_tid = INT32_MIN, prev = I.last_tid_seen;
        bool saw_unmapped = false;
        while (o + 4 <= buf.size()) {
            uint32_t bs; memcpy(&bs, buf.data() + o, 4);
            if (bs < 32) throw Error(FLORIA_E_INVALID, I.path + ": malformed BAM record");
            if (o + 4 + (size_t)bs > buf.size()) break;
            int32_t tid; memcpy(&tid, buf.data() + o + 4, 4);
            if (tid < 0) { if (!saw_unmapped) { saw_unmapped = true; last_start_of_tid = o; cur_tid = n_targets; } }      // unplaced reads close the file: every target is complete
            else if (saw_unmapped || tid < prev) throw Error(FLORIA_E_INVALID, I.path + " is not sorted by reference sequence (floria needs a coordinate-sorted, indexed BAM; so does this reader)");
            else if (tid != cur_tid) { cur_tid = tid; last_start_of_tid = o; prev = tid; }
            o += 4 + (size_t)bs;
            whole_end = o;
        }
        if (at_end && whole_end != buf.size()) throw Error(FLORIA_E_INVALID, I.path + " is truncated");
        // Unplaced reads (tid = -1) sort behind every target: once one is seen, every target is complete and nothing that follows is of use (the reference fetches
        // per contig through the index and never reads them, file_reader.rs:389-436).  The stream ends there — carrying an unmapped tail larger than the window
        // from call to call would never make progress.
        const bool closing = at_end || saw_unmapped;
        size_t cut; int32_t complete_upto;
        if (closing) { cut = saw_unmapped ? last_start_of_tid : whole_end; complete_upto = n_targets; }
        else { cut = last_start_of_tid; complete_upto = cur_tid == INT32_MIN ? I.done_upto : std::min(cur_tid, n_targets); }      // the target of the last record may continue
        if (!closing && (cut == 0 || complete_upto <= I.done_upto)) { want = std::max(want * 2, buf.size() * 2); continue; }   // one target fills the buffer: read on
        // ---- hand out
        seg = BamFile();
        seg.target_names = I.names; seg.target_len = I.lens;
        seg.by_tid.resize(I.names.size());
        I.carry.assign(buf.begin() + (ptrdiff_t)cut, buf.begin() + (ptrdiff_t)(closing ? cut : buf.size()));
        buf.resize(cut);
        seg.raw = std::move(buf);
        I.peak = std::max(I.peak, seg.raw.size() + I.carry.size());
        decode_records(seg, 0, seg.raw.size(), I.path, I.threads);
        seg.tid_begin = I.done_upto; seg.tid_end = complete_upto;
        I.done_upto = complete_upto;
        I.last_tid_seen = std::max(I.last_tid_seen, std::min(prev, n_targets));
        if (closing) { I.eof = true; I.carry.clear(); }
        return true;
    }
}

std::vector<std::string> get_contigs_to_phase(const BamFile& bam) { return bam.target_names; }

// get_vcf_profile + get_genotypes_from_vcf_hts (file_reader.rs:113-175, 239-314).  rust-htslib's bcf::Reader takes text VCF (plain / gzip / bgzip) and binary
// BCF2 alike; so does this reader: the file is read through zlib (a BGZF file is a multi-member gzip stream) and told apart by its first bytes.
namespace {
struct VcfSink {
    VcfProfile vp;
    const std::vector<std::string>& ref_chroms;
    std::string last_chrom;
    bool have_last = false;
    SnpPosition snp_counter = 1;
    explicit VcfSink(const std::vector<std::string>& rc) : ref_chroms(rc) {}
    static bool is_acgt(char ch) { const char u = (char)(ch & ~0x20); return u == 'A' || u == 'C' || u == 'G' || u == 'T'; }
    // one record: CHROM, 1-based POS, REF + ALT alleles
    void add(const std::string& chrom, long pos1, const std::vector<std::string>& alleles) {
        const bool known = std::find(ref_chroms.begin(), ref_chroms.end(), chrom) != ref_chroms.end();
        if (known && (!have_last || last_chrom != chrom)) { snp_counter = 1; last_chrom = chrom; have_last = true; }       // :277-280
        std::vector<Genotype> al_vec;
        for (const std::string& a : alleles) {
            if (a.size() != 1 || !is_acgt(a[0])) return;                                                                   // :290-300 (an empty allele cannot occur)
            al_vec.push_back((Genotype)a[0]);
        }
        const GnPosition pos0 = (GnPosition)(pos1 - 1);                          // htslib's 0-based pos()
        vp.snp_to_genome_pos[chrom].push_back(pos0);                             // get_genotypes_from_vcf_hts: every contig of the VCF
        if (!known) return;
        vp.vcf_snp_pos_to_gn_pos_map[chrom][snp_counter] = pos0;
        vp.vcf_pos_to_snp_counter_map[chrom][pos0] = snp_counter;
        vp.vcf_pos_allele_map[chrom][pos0] = al_vec;
        ++snp_counter;
    }
};

// BCF2 (VCFv4.x specification, section 6): "BCF\2\2", l_text, the VCF header text, then records {l_shared, l_indiv, CHROM (index into the header's contig
// dictionary), POS (0-based), rlen, QUAL, n_info | n_allele << 16, n_sample | n_fmt << 24, ID, alleles ..}: typed values with a descriptor byte
// (length << 4 | type; length 15 = a typed integer with the real length follows; type 7 = characters).  Only CHROM, POS and the alleles are read.
void read_bcf(gzFile f, const std::string& vcf_file, std::vector<unsigned char> head, VcfSink& sink) {
    auto fail = [&](const char* what) -> void { throw Error(FLORIA_E_INVALID, "BCF " + vcf_file + ": " + what); };
    auto need = [&](std::vector<unsigned char>& buf, size_t n) {
        const size_t have = buf.size();
        if (have >= n) return true;
        buf.resize(n);
        size_t got = have;
        while (got < n) { const int r = gzread(f, buf.data() + got, (unsigned)std::min<size_t>(n - got, 1u << 30)); if (r <= 0) break; got += (size_t)r; }
        buf.resize(got);
        return got >= n;
    };
    auto u32 = [](const unsigned char* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; };
    if (!need(head, 9) || memcmp(head.data(), "BCF\2", 4) != 0 || head[4] < 1) fail("not a BCF2 file");
    const uint32_t l_text = u32(head.data() + 5);
    if (!need(head, 9 + (size_t)l_text)) fail("truncated header");
    // the contig dictionary: ##contig=<ID=name,..[,IDX=k]> lines in order (IDX overrides the position)
    std::vector<std::string> contigs;
    {
        const std::string text((const char*)head.data() + 9, l_text);
        size_t at = 0;
        while (at < text.size()) {
            size_t e = text.find('\n', at); if (e == std::string::npos) e = text.size();
            const std::string line = text.substr(at, e - at);
            at = e + 1;
            if (line.rfind("##contig=<", 0) != 0) continue;
            std::string id; long idx = -1;
            size_t q = 10;
            while (q < line.size() && line[q] != '>') {
                size_t eq = line.find('=', q), stop = q;
                if (eq == std::string::npos) break;
                const std::string key = line.substr(q, eq - q);
                size_t v0 = eq + 1, v1;
                if (v0 < line.size() && line[v0] == '"') { v1 = line.find('"', v0 + 1); if (v1 == std::string::npos) v1 = line.size(); stop = v1 + 1; ++v0; }
                else { v1 = line.find_first_of(",>", v0); if (v1 == std::string::npos) v1 = line.size(); stop = v1; }
                const std::string val = line.substr(v0, v1 - v0);
                if (key == "ID") id = val; else if (key == "IDX") idx = strtol(val.c_str(), nullptr, 10);
                q = stop; if (q < line.size() && line[q] == ',') ++q;
            }
            if (id.empty()) continue;
            if (idx < 0) idx = (long)contigs.size();
            if ((size_t)idx >= contigs.size()) contigs.resize((size_t)idx + 1);
            contigs[(size_t)idx] = id;
        }
    }
    std::vector<unsigned char> rec;
    for (;;) {
        rec.clear();
        if (!need(rec, 8)) { if (rec.empty()) break; fail("truncated record header"); }
        const uint32_t l_shared = u32(rec.data()), l_indiv = u32(rec.data() + 4);
        if (l_shared < 24) fail("record shorter than its fixed fields");
        // only the shared part is parsed: it is bounded (a corrupt or hostile length must become a floria Error, not a bad_alloc), the per-sample part is skipped
        // in bounded reads instead of being buffered
        if (l_shared > (64u << 20)) fail("record with a shared part of more than 64 MB");
        rec.clear();
        if (!need(rec, (size_t)l_shared)) fail("truncated record");
        {
            unsigned char skip[1 << 16];
            for (uint64_t left = l_indiv; left != 0;) {
                const int r = gzread(f, skip, (unsigned)std::min<uint64_t>(left, sizeof skip));
                if (r <= 0) fail("truncated record");
                left -= (uint64_t)r;
            }
        }
        const unsigned char* q = rec.data();
        const unsigned char* const end = q + l_shared;
        const int32_t chrom = (int32_t)u32(q), pos0 = (int32_t)u32(q + 4);
        const uint32_t n_allele = u32(q + 16) >> 16;
        q += 24;
        if (chrom < 0 || (size_t)chrom >= contigs.size() || contigs[(size_t)chrom].empty()) fail("CHROM index outside the header's contig dictionary");
        // typed value: -> (type, count), cursor behind the descriptor
        auto typed = [&](uint32_t& type, uint32_t& count) {
            if (q >= end) fail("typed value beyond the record");
            const unsigned d = *q++;
            type = d & 15u; count = d >> 4;
            if (count == 15) {                                        // the real length is a typed integer
                if (q >= end) fail("typed length beyond the record");
                const unsigned t2 = *q++ & 15u;
                const size_t w = t2 == 1 ? 1 : t2 == 2 ? 2 : t2 == 3 ? 4 : 0;
                if (!w || q + w > end) fail("bad typed length");
                count = w == 1 ? q[0] : w == 2 ? (uint32_t)q[0] | (uint32_t)q[1] << 8 : u32(q);
                q += w;
            }
        };
        auto width = [&](uint32_t type) -> size_t { return type == 1 || type == 7 ? 1 : type == 2 ? 2 : type == 3 || type == 5 ? 4 : 0; };
        uint32_t ty, cnt;
        typed(ty, cnt);                                                // ID
        if (cnt && (!width(ty) || q + (size_t)cnt * width(ty) > end)) fail("bad ID");
        q += (size_t)cnt * width(ty);
        std::vector<std::string> alleles;
        for (uint32_t a = 0; a < n_allele; ++a) {
            typed(ty, cnt);
            if (cnt && (ty != 7 || q + cnt > end)) fail("allele is not a string");
            alleles.emplace_back((const char*)q, cnt);
            q += cnt;
        }
        if (alleles.empty()) continue;
        sink.add(contigs[(size_t)chrom], (long)pos0 + 1, alleles);
    }
}
}  // namespace

VcfProfile get_vcf_profile(const std::string& vcf_file, const std::vector<std::string>& ref_chroms) {
    gzFile f = gzopen(vcf_file.c_str(), "rb");                                 // plain text, gzip and bgzip alike
    if (!f) throw Error(FLORIA_E_INVALID, "cannot open VCF " + vcf_file);
    VcfSink sink(ref_chroms);
    std::vector<char> buf(1 << 16);
    {   // BCF2 or text?
        std::vector<unsigned char> head(5);
        const int got = gzread(f, head.data(), 5);
        head.resize(got > 0 ? (size_t)got : 0);
        if (head.size() == 5 && memcmp(head.data(), "BCF\2", 4) == 0) {
            try { read_bcf(f, vcf_file, std::move(head), sink); } catch (...) { gzclose(f); throw; }
            gzclose(f);
            return std::move(sink.vp);
        }
        if (gzrewind(f) != 0) { gzclose(f); throw Error(FLORIA_E_INVALID, "cannot rewind VCF " + vcf_file); }
    }
    std::string line;
    for (;;) {
        line.clear();
        bool got = false;
        while (gzgets(f, buf.data(), (int)buf.size())) { got = true; line += buf.data(); if (!line.empty() && line.back() == '\n') break; }
        if (!got) break;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        // CHROM POS ID REF ALT ...
        size_t t[5], k = 0, from = 0;
        while (k < 5) { const size_t x = line.find('\t', from); if (x == std::string::npos) break; t[k++] = x; from = x + 1; }
        if (k < 4) continue;
        const std::string chrom = line.substr(0, t[0]);
        const long pos1 = strtol(line.c_str() + t[0] + 1, nullptr, 10);
        const std::string ref = line.substr(t[2] + 1, t[3] - t[2] - 1);
        const std::string alt = line.substr(t[3] + 1, (k == 5 ? t[4] : line.size()) - t[3] - 1);
        std::vector<std::string> alleles{ref};
        if (alt != ".") { size_t a = 0; for (;;) { const size_t x = alt.find(',', a); alleles.push_back(alt.substr(a, x == std::string::npos ? x : x - a)); if (x == std::string::npos) break; a = x + 1; } }
        sink.add(chrom, pos1, alleles);
    }
    gzclose(f);
    return std::move(sink.vp);
}

std::map<std::string, std::string> get_fasta_seqs(const std::string& fasta_file) {
    gzFile f = gzopen(fasta_file.c_str(), "rb");
    if (!f) throw Error(FLORIA_E_INVALID, "Could not read fasta file " + fasta_file);
    std::map<std::string, std::string> out;
    std::string* cur = nullptr;
    std::vector<char> buf(1 << 16);
    while (gzgets(f, buf.data(), (int)buf.size())) {
        size_t n = strlen(buf.data());
        while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) --n;
        if (n && buf[0] == '>') {
            size_t e = 1;
            while (e < n && buf[e] != ' ' && buf[e] != '\t') ++e;
            cur = &out[std::string(buf.data() + 1, e - 1)];
        } else if (cur) cur->append(buf.data(), n);
    }
    gzclose(f);
    return out;
}

struct ContigIngest::Impl {
    std::vector<std::vector<Tagged>> buckets;                                  // read name -> its passing alignments, in record order
    const std::map<SnpPosition, GnPosition>* snp_to_gn = nullptr;
    int64_t supp_aln_dist_cutoff = 0;
    size_t n_records = 0;                                                      // of the contig, passing or not: the Frags' counter_ids lie below it
};
ContigIngest::~ContigIngest() = default;
ContigIngest::ContigIngest(ContigIngest&&) noexcept = default;
ContigIngest& ContigIngest::operator=(ContigIngest&&) noexcept = default;

ContigIngest::ContigIngest(const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string& contig, const std::string* ref_seq, RealignQueue* queue,
                           const RecordPileup* device_cells)
    : p_(new Impl) {
    const bool filter_supplementary = true, use_supplementary = !o.dont_use_supp_aln;
    const auto tid_it = std::find(bam.target_names.begin(), bam.target_names.end(), contig);
    if (tid_it == bam.target_names.end()) return;
    const int32_t tid = (int32_t)(tid_it - bam.target_names.begin());
    const auto& snp_positions = vp.vcf_pos_to_snp_counter_map.at(contig);
    const auto& pos_allele_map = vp.vcf_pos_allele_map.at(contig);
    const auto& snp_to_gn = vp.vcf_snp_pos_to_gn_pos_map.at(contig);
    p_->snp_to_gn = &snp_to_gn; p_->supp_aln_dist_cutoff = o.supp_aln_dist_cutoff;
    // read name -> its passing alignments, in record order (the reference fills the buckets from a parallel loop)
    std::vector<std::string> names;
    std::unordered_map<std::string, size_t> name_ix;
    std::vector<std::vector<Tagged>>& buckets = p_->buckets;
    size_t count = 0;
    for (const uint32_t rec_ix : bam.by_tid[tid]) {                           // the contig's records in file order, as fetch() yields them
        const BamRecord& rec = bam.records[rec_ix];
        const size_t this_count = count++;
        if (!alignment_passed_check(rec.flags, rec.mapq, use_supplementary, filter_supplementary, o.mapq_cutoff).first) continue;
        auto ins = name_ix.emplace(std::string(rec.qname), names.size());
        if (ins.second) { names.emplace_back(rec.qname); buckets.emplace_back(); }
        RecordPileup::Cells dc;
        const bool on_device = device_cells && device_cells->cells(rec_ix, dc);
        Frag fr = on_device ? frag_from_cells(rec, dc, this_count, o.output_reads) : frag_from_record(rec, snp_positions, pos_allele_map, this_count, o.output_reads);
        if (ref_seq && !(on_device && device_cells->realigned)) realign(*ref_seq, fr, rec.seq, snp_to_gn, pos_allele_map, queue, o.realign_walk ? &o.walk : nullptr);             // :416-423
        buckets[ins.first->second].push_back({rec.flags, std::move(fr), rec_ix});
    }
    p_->n_records = count;
}

// ---- --pileup device ------------------------------------------------------------------------------------------------------------------------
RecordPileup::~RecordPileup() { floria_hip_record_cells_free(cells_); }
bool RecordPileup::cells(uint32_t rec_ix, Cells& out) const {
    const uint32_t s = rec_ix < slot_.size() ? slot_[rec_ix] : 0;
    if (!s) return false;
    const uint64_t b = cells_->cell_off[s - 1], e = cells_->cell_off[s];
    out = {cells_->snp + b, cells_->allele + b, cells_->qual + b, cells_->seq_pos + b, (size_t)(e - b), cells_->ref_end[s - 1]};
    return true;
}
// The records of a round that go to the device, as floria_hip_pileup_records* takes them (shared by --pileup device / fused / resident): every record of the given
// contigs that passes alignment_passed_check, as offsets into the stretch of the segment's inflated buffer that holds them; the SNP table of those contigs; with
// ref_seqs their reference sequences back to back.  A contig the device's numbering (rank + 1) would not match, or with a site of more than FLORIA_MAX_ALLELES
// alleles, is not sent (host_contigs).
struct RecordSelection {
    std::vector<uint64_t> snp_off{0};
    std::vector<int64_t> snp_pos;
    std::vector<uint8_t> alleles, n_alleles;
    std::vector<int32_t> pos;
    std::vector<uint16_t> flags;
    std::vector<uint32_t> contig, n_cigar, l_seq, rec_of;
    std::vector<uint64_t> cigar_off, seq_off, qual_off;
    std::vector<uint64_t> ref_off{0};                                          // ref_seqs: the table's contigs' sequences back to back
    std::vector<uint8_t> ref_bytes;
    std::vector<std::string> host_contigs;
    std::vector<int32_t> table_of;                                             // contig of the list -> contig of the table, -1: not sent
    size_t blob_bytes = 0;
    floria_alignments A{};
    floria_snp_table S{};
    floria_ref_seqs F{};
    size_t n() const { return pos.size(); }
    RecordSelection(const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string* contigs, size_t n_contigs, const std::map<std::string, std::string>* ref_seqs) {
        const bool filter_supplementary = true, use_supplementary = !o.dont_use_supp_aln;
        std::vector<const unsigned char*> cig_p, seq_p, qual_p;
        table_of.assign(n_contigs, -1);
        for (size_t ci = 0; ci < n_contigs; ++ci) {
            const auto tid_it = std::find(bam.target_names.begin(), bam.target_names.end(), contigs[ci]);
            const auto counters = vp.vcf_pos_to_snp_counter_map.find(contigs[ci]);
            const auto pam = vp.vcf_pos_allele_map.find(contigs[ci]);
            if (tid_it == bam.target_names.end() || counters == vp.vcf_pos_to_snp_counter_map.end() || pam == vp.vcf_pos_allele_map.end()) continue;
            // both maps in lockstep: the same positions, the counters 1, 2, .. in position order, 1 to FLORIA_MAX_ALLELES alleles at every site
            bool ok = counters->second.size() == pam->second.size();
            SnpPosition rank = 0;
            auto al = pam->second.begin();
            for (auto ct = counters->second.begin(); ok && ct != counters->second.end(); ++ct, ++al)
                ok = ct->first == al->first && ct->second == ++rank && !al->second.empty() && al->second.size() <= FLORIA_MAX_ALLELES;
            if (!ok) { host_contigs.push_back(contigs[ci]); continue; }
            const uint32_t table_ix = (uint32_t)snp_off.size() - 1;
            table_of[ci] = (int32_t)table_ix;
            for (const auto& kv : pam->second) {
                snp_pos.push_back((int64_t)kv.first);
                for (size_t a = 0; a < FLORIA_MAX_ALLELES; ++a) alleles.push_back(a < kv.second.size() ? kv.second[a] : 0);
                n_alleles.push_back((uint8_t)kv.second.size());
            }
            snp_off.push_back(snp_pos.size());
            if (ref_seqs) {
                const auto fa = ref_seqs->find(contigs[ci]);
                if (fa != ref_seqs->end()) ref_bytes.insert(ref_bytes.end(), fa->second.begin(), fa->second.end());
                ref_off.push_back(ref_bytes.size());
            }
            for (const uint32_t rec_ix : bam.by_tid[(size_t)(tid_it - bam.target_names.begin())]) {
                const BamRecord& rec = bam.records[rec_ix];
                if (!alignment_passed_check(rec.flags, rec.mapq, use_supplementary, filter_supplementary, o.mapq_cutoff).first) continue;
                pos.push_back(rec.pos); flags.push_back(rec.flags); contig.push_back(table_ix); n_cigar.push_back((uint32_t)rec.cigar.n); l_seq.push_back((uint32_t)rec.seq.n);
                cig_p.push_back(rec.cigar.p); seq_p.push_back(rec.seq.packed); qual_p.push_back(rec.qual.p); rec_of.push_back(rec_ix);
            }
        }
        const size_t n = pos.size();
        if (n == 0) return;
        // the stretch of the inflated buffer that holds these records' CIGARs, bases and qualities (a round's contigs are neighbours in a sorted BAM)
        // (a device segment: the views hold blob offsets already, the blob is the segment's handle and nothing travels)
        uintptr_t lo = 0, hi = 0;
        if (bam.dev) hi = (uintptr_t)floria_hip_blob_bytes(bam.dev->blob);
        else {
            lo = hi = (uintptr_t)cig_p[0];
            for (size_t i = 0; i < n; ++i) {
                lo = std::min({lo, (uintptr_t)cig_p[i], (uintptr_t)seq_p[i], (uintptr_t)qual_p[i]});
                hi = std::max({hi, (uintptr_t)cig_p[i] + 4 * (size_t)n_cigar[i], (uintptr_t)seq_p[i] + ((size_t)l_seq[i] + 1) / 2, (uintptr_t)qual_p[i] + l_seq[i]});
            }
        }
        cigar_off.resize(n); seq_off.resize(n); qual_off.resize(n);
        for (size_t i = 0; i < n; ++i) { cigar_off[i] = (uint64_t)((uintptr_t)cig_p[i] - lo); seq_off[i] = (uint64_t)((uintptr_t)seq_p[i] - lo); qual_off[i] = (uint64_t)((uintptr_t)qual_p[i] - lo); }
        blob_bytes = (size_t)(hi - lo);
        A.blob = bam.dev ? nullptr : (const uint8_t*)lo; A.blob_bytes = blob_bytes; A.n_records = (uint32_t)n; A.pos = pos.data(); A.flags = flags.data(); A.contig = contig.data();
        A.cigar_off = cigar_off.data(); A.n_cigar = n_cigar.data(); A.seq_off = seq_off.data(); A.l_seq = l_seq.data(); A.qual_off = qual_off.data();
        S.n_contigs = (uint32_t)snp_off.size() - 1; S.snp_off = snp_off.data(); S.snp_pos = snp_pos.data(); S.alleles = alleles.data(); S.n_alleles = n_alleles.data();
        F.n_contigs = S.n_contigs; F.seq_off = ref_off.data(); F.seq = ref_bytes.data();
    }
    RecordSelection(const RecordSelection&) = delete;
    RecordSelection& operator=(const RecordSelection&) = delete;
};

void RoundWalk::walk(Session& session, const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string* contigs, size_t n_contigs,
                     const std::map<std::string, std::string>* ref_seqs, const std::function<void(const RecordSelection&)>& call) {
    RecordSelection sel(bam, vp, o, contigs, n_contigs, ref_seqs);
    host_contigs = sel.host_contigs;
    table_of_ = sel.table_of;
    for (size_t c = 0; c + 1 < sel.snp_off.size(); ++c) snp_count_.push_back(sel.snp_off[c + 1] - sel.snp_off[c]);
    const size_t n = sel.n();
    records_sent = n;
    if (n == 0) return;
    blob_bytes = sel.blob_bytes;
    call(sel);
    floria_timing tm;
    if (floria_hip_last_timing(session.ctx(), &tm) == 0) { kernel_ms = tm.pileup_ms; h2d_ms = tm.h2d_ms; d2h_ms = tm.d2h_ms; }
    slot_.assign(bam.records.size(), 0);
    for (size_t i = 0; i < n; ++i) slot_[sel.rec_of[i]] = (uint32_t)i + 1;
}

RecordPileup::RecordPileup(Session& session, const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string* contigs, size_t n_contigs,
                           const std::map<std::string, std::string>* ref_seqs) {
    walk(session, bam, vp, o, contigs, n_contigs, ref_seqs, [&](const RecordSelection& sel) {
        if (ref_seqs) {
            if (const int rc = floria_hip_pileup_records_realign(session.ctx(), &sel.A, &sel.S, &sel.F, o.realign_walk ? &o.walk : nullptr, &cells_, &counts))
                throw Error(rc, std::string("floria_hip_pileup_records_realign: ") + floria_hip_last_error());
            realigned = true;
        } else if (const int rc = floria_hip_pileup_records(session.ctx(), &sel.A, &sel.S, &cells_)) throw Error(rc, std::string("floria_hip_pileup_records: ") + floria_hip_last_error());
    });
}

// ---- combine_frags on headers (every route) ------------------------------------------------------------------------------------------------------
// The decisions of combine_frags (:491-659) on (flags, counter_id, first, last) alone: ContigIngest::finish() merges its Frags by this plan, --pileup resident hands
// it to the device.  A record without cells has first = UINT32_MAX and last = 0, what its Frag has, so the sort of a pair, the intervals of a supplementary group and
// the merged ends come out as they do on the Frags themselves.
ContigPlan plan_contig(std::vector<std::vector<PlanRecord>>& groups, const std::map<SnpPosition, GnPosition>& snp_to_gn, int64_t supp_aln_dist_cutoff) {
    const auto frag_less = [](SnpPosition af, SnpPosition al, size_t ac, SnpPosition bf, SnpPosition bl, size_t bc) {      // Frag::cmp
        if (af != bf) return af < bf;
        if (al != bl) return al > bl;
        return ac < bc;
    };
    const auto paired = [](const PlanRecord& r) { return (r.flags & F_PAIRED1) || (r.flags & F_PAIRED2); };
    ContigPlan out;
    for (auto& g : groups) {
        PlannedFrag pf;
        if (g.size() == 2 && paired(g[0]) && paired(g[1])) {
            std::sort(g.begin(), g.end(), [&](const PlanRecord& a, const PlanRecord& b) {
                return a.flags != b.flags ? a.flags < b.flags : frag_less(a.first, a.last, a.counter_id, b.first, b.last, b.counter_id);
            });
            size_t ff, sf;
            if ((g[0].flags & F_PAIRED1) == F_PAIRED1) { ff = 0; sf = 1; }
            else if ((g[0].flags & F_PAIRED2) == F_PAIRED2) { ff = 1; sf = 0; }
            else continue;
            pf.parts = {g[ff], g[sf]}; pf.mate = {0, 1};
        } else if (g.size() == 1 && (g[0].flags & F_SUPP) == 0) {
            pf.parts = {g[0]}; pf.mate = {0};
        } else {
            std::vector<std::pair<SnpPosition, SnpPosition>> supp_intervals;
            for (const PlanRecord& r : g) if (r.has_cells()) supp_intervals.push_back({r.first, r.last});
            std::sort(supp_intervals.begin(), supp_intervals.end());
            bool take_primary_only = false;
            for (size_t i = 0; i + 1 < supp_intervals.size(); ++i)
                if ((int64_t)snp_to_gn.at(supp_intervals[i + 1].first) - (int64_t)snp_to_gn.at(supp_intervals[i].second) > supp_aln_dist_cutoff) { take_primary_only = true; break; }
            int primary = -1;
            for (size_t i = 0; i < g.size(); ++i) if ((g[i].flags & F_SUPP) != F_SUPP) primary = (int)i;             // the LAST primary wins (:606-614)
            if (primary < 0) continue;                                                                              // supplementary records only
            pf.parts.push_back(g[(size_t)primary]);
            if (!take_primary_only) for (size_t i = 0; i < g.size(); ++i) if ((int)i != primary) pf.parts.push_back(g[i]);
            pf.mate.assign(pf.parts.size(), 0);
        }
        for (const PlanRecord& r : pf.parts) { pf.first = std::min(pf.first, r.first); pf.last = std::max(pf.last, r.last); }
        pf.counter_id = pf.parts[0].counter_id;
        (pf.first == UINT32_MAX ? out.snpless : out.frags).push_back(std::move(pf));
    }
    std::sort(out.frags.begin(), out.frags.end(), [&](const PlannedFrag& a, const PlannedFrag& b) { return frag_less(a.first, a.last, a.counter_id, b.first, b.last, b.counter_id); });
    return out;
}

std::string plan_text(const std::string& contig, const ContigPlan& plan, const BamFile& bam) {
    std::string t = "#CONTIG\t" + contig + "\t" + std::to_string(plan.frags.size()) + "\t" + std::to_string(plan.snpless.size()) + "\n";
    const auto parts = [&](const PlannedFrag& f) {
        for (size_t k = 0; k < f.parts.size(); ++k) {
            const BamRecord& r = bam.records[f.parts[k].rec];
            t += "\t" + std::string(r.qname) + ":" + std::to_string(r.flags) + ":" + std::to_string(r.pos) + ":" + std::to_string((int)f.mate[k]);
        }
        t += "\n";
    };
    for (const PlannedFrag& f : plan.frags) {
        t += "F\t" + std::string(bam.records[f.parts[0].rec].qname) + "\t" + std::to_string(f.first) + "\t" + std::to_string(f.last);
        parts(f);
    }
    for (const PlannedFrag& f : plan.snpless) { t += "S\t" + std::string(bam.records[f.parts[0].rec].qname); parts(f); }
    return t;
}

ContigPlan ContigIngest::plan() const {
    if (p_->buckets.empty()) return {};
    std::vector<std::vector<PlanRecord>> groups(p_->buckets.size());
    for (size_t b = 0; b < groups.size(); ++b)
        for (const Tagged& t : p_->buckets[b]) {
            PlanRecord r;
            r.rec = t.rec_ix; r.flags = t.flags; r.counter_id = t.frag.counter_id; r.first = t.frag.first_position; r.last = t.frag.last_position;
            groups[b].push_back(r);
        }
    return plan_contig(groups, *p_->snp_to_gn, p_->supp_aln_dist_cutoff);
}

namespace {
// first_frag.positions.extend(..) and what goes with it (:539-562 for a mate, :633-650 for a supplementary piece): `fr` is merged onto `base`
void extend_frag(Frag& base, Frag& fr, bool mate) {
    if (!fr.seq_dict.empty()) {                                                        // positions.extend (:541, :639): remember who brought what
        base.merged_positions = true;
        if (base.position_segments.empty()) { base.position_segments.emplace_back(); for (const auto& kv : base.seq_dict) base.position_segments[0].push_back(kv.first); }
        base.position_segments.emplace_back();
        for (const auto& kv : fr.seq_dict) base.position_segments.back().push_back(kv.first);
    }
    for (auto& kv : fr.seq_dict) base.seq_dict[kv.first] = kv.second;                  // extend: the later part's call overwrites
    for (auto& kv : fr.qual_dict) base.qual_dict[kv.first] = kv.second;
    base.first_position = std::min(base.first_position, fr.first_position);
    base.last_position = std::max(base.last_position, fr.last_position);
    base.first_pos_base = std::min(base.first_pos_base, fr.first_pos_base);
    base.last_pos_base = std::min(base.last_pos_base, fr.last_pos_base);               // (min, as in the reference, :547)
    if (mate) {
        base.seq_len[1] = fr.seq_len[0];
        base.seq_string[1] = std::move(fr.seq_string[0]); base.qual_string[1] = std::move(fr.qual_string[0]);   // :551-554
        for (auto& kv : fr.snp_pos_to_seq_pos) base.snp_pos_to_seq_pos[kv.first] = {1, kv.second.second};
    } else
        for (auto& kv : fr.snp_pos_to_seq_pos) base.snp_pos_to_seq_pos[kv.first] = kv.second;
}
}  // namespace

std::pair<std::vector<Frag>, std::vector<Frag>> ContigIngest::finish() {
    std::vector<std::vector<Tagged>>& buckets = p_->buckets;
    if (buckets.empty()) return {};
    const ContigPlan pl = plan();
    std::vector<Frag*> by_counter(p_->n_records, nullptr);                             // a part is named by its counter_id: the record's place among the contig's
    for (auto& frags : buckets) for (Tagged& t : frags) by_counter[t.frag.counter_id] = &t.frag;
    const auto merged = [&](const PlannedFrag& pf) -> Frag& {
        Frag& base = *by_counter[pf.parts[0].counter_id];
        for (size_t k = 1; k < pf.parts.size(); ++k) extend_frag(base, *by_counter[pf.parts[k].counter_id], pf.mate[k] != 0);
        return base;
    };
    std::pair<std::vector<Frag>, std::vector<Frag>> out;
    out.first.reserve(pl.frags.size()); out.second.reserve(pl.snpless.size());
    for (const PlannedFrag& pf : pl.frags) out.first.push_back(std::move(merged(pf)));
    for (const PlannedFrag& pf : pl.snpless) out.second.push_back(std::move(merged(pf)));
    buckets.clear();
    return out;
}

ResidentPileup::~ResidentPileup() { floria_hip_record_summary_free(summary_); }
ResidentPileup::ResidentPileup(Session& session, const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string* contigs, size_t n_contigs,
                               const std::map<std::string, std::string>* ref_seqs)
    : s_(session), bam_(bam), vp_(vp), o_(o), contigs_(contigs) {
    walk(session, bam, vp, o, contigs, n_contigs, ref_seqs, [&](const RecordSelection& sel) {
        if (bam.dev) {                                                         // the records lie in the segment's blob: nothing is uploaded
            if (const int rc = floria_hip_pileup_records_resident_blob(session.ctx(), bam.dev->blob, &sel.A, &sel.S, ref_seqs ? &sel.F : nullptr, o.realign_walk ? &o.walk : nullptr, &summary_))
                throw Error(rc, std::string("floria_hip_pileup_records_resident_blob: ") + floria_hip_last_error());
        } else if (const int rc = floria_hip_pileup_records_resident(session.ctx(), &sel.A, &sel.S, ref_seqs ? &sel.F : nullptr, o.realign_walk ? &o.walk : nullptr, &summary_))
            throw Error(rc, std::string("floria_hip_pileup_records_resident: ") + floria_hip_last_error());
        counts = summary_->counts;
        bytes_back += (uint64_t)sel.n() * 24 + 8;                              // cell_off, first_snp, last_snp, ref_end
    });
}

HeaderContig ResidentPileup::plan(size_t ci) const {
    HeaderContig hc;
    if (!summary_ || table_of_[ci] < 0) return hc;
    const std::string& contig = contigs_[ci];
    const auto tid_it = std::find(bam_.target_names.begin(), bam_.target_names.end(), contig);
    if (tid_it == bam_.target_names.end()) return hc;
    const bool filter_supplementary = true, use_supplementary = !o_.dont_use_supp_aln;
    // read name -> its passing alignments in record order, as ContigIngest buckets them
    std::unordered_map<std::string_view, size_t> name_ix;
    std::vector<std::vector<PlanRecord>> groups;
    size_t count = 0;
    for (const uint32_t rec_ix : bam_.by_tid[(size_t)(tid_it - bam_.target_names.begin())]) {
        const BamRecord& rec = bam_.records[rec_ix];
        const size_t this_count = count++;
        if (!alignment_passed_check(rec.flags, rec.mapq, use_supplementary, filter_supplementary, o_.mapq_cutoff).first) continue;
        const uint32_t s = slot_[rec_ix];
        if (!s) throw Error(FLORIA_E_INVALID, "resident pileup: a passing record of contig " + contig + " was not sent");
        auto ins = name_ix.emplace(rec.qname, groups.size());
        if (ins.second) groups.emplace_back();
        PlanRecord r;
        r.rec = rec_ix; r.flags = rec.flags; r.counter_id = this_count;
        if (summary_->cell_off[s] > summary_->cell_off[s - 1]) { r.first = summary_->first_snp[s - 1]; r.last = summary_->last_snp[s - 1]; }
        groups[ins.first->second].push_back(r);
    }
    hc.plan = plan_contig(groups, vp_.vcf_snp_pos_to_gn_pos_map.at(contig), o_.supp_aln_dist_cutoff);
    // the header Frag of a planned fragment: the base's identity, the ends combine_frags gives the merged one, the second mate's bases where there is one
    const auto header = [&](const PlanRecord& r, bool keep_sequences) {
        const BamRecord& rec = bam_.records[r.rec];
        Frag f = frag_without_calls(rec, r.counter_id);
        f.last_pos_base = (GnPosition)summary_->ref_end[slot_[r.rec] - 1];
        frag_sequences(f, rec, keep_sequences && !bam_.dev);                   // (a device segment's bases come in one call for the round: fetch_sequences)
        return f;
    };
    const auto merged = [&](const PlannedFrag& pf, bool with_cells) {
        Frag f = header(pf.parts[0], o_.output_reads);
        size_t parts_with_cells = pf.parts[0].has_cells() ? 1 : 0;
        for (size_t k = 1; k < pf.parts.size(); ++k) {
            Frag g = header(pf.parts[k], o_.output_reads && pf.mate[k]);
            f.first_pos_base = std::min(f.first_pos_base, g.first_pos_base);
            f.last_pos_base = std::min(f.last_pos_base, g.last_pos_base);                  // (min, as in the reference, :547)
            if (pf.mate[k]) { f.seq_len[1] = g.seq_len[0]; f.seq_string[1] = std::move(g.seq_string[0]); f.qual_string[1] = std::move(g.qual_string[0]); }
            if (pf.parts[k].has_cells()) { f.merged_positions = true; ++parts_with_cells; }
        }
        f.first_position = pf.first; f.last_position = pf.last;
        if (with_cells) {
            if (parts_with_cells >= 2) ++hc.merged_frags;
            for (const PlanRecord& r : pf.parts) { const uint32_t s = slot_[r.rec]; hc.part_cells += summary_->cell_off[s] - summary_->cell_off[s - 1]; }
        }
        return f;
    };
    hc.all_frags.reserve(hc.plan.frags.size());
    for (const PlannedFrag& pf : hc.plan.frags) { hc.all_frags.push_back(merged(pf, true)); hc.all_frags.back().counter_id = hc.all_frags.size() - 1; }
    for (const PlannedFrag& pf : hc.plan.snpless) hc.frags_without_snps.push_back(merged(pf, false));
    return hc;
}

void ResidentPileup::assemble(std::vector<HeaderContig*>& planned, bool derive_set_order, bool keep_seq_pos, bool ignore_monomorphic, double epsilon) {
    if (!summary_) return;                                                                 // nothing was sent: no contig of the round has a fragment
    fetch_sequences(planned);                                                              // (before the filter below re-orders the Frags)
    const size_t nt = snp_count_.size();
    std::vector<HeaderContig*> by_table(nt, nullptr);
    for (size_t ci = 0; ci < planned.size(); ++ci) if (table_of_[ci] >= 0) by_table[(size_t)table_of_[ci]] = planned[ci];
    std::vector<uint64_t> frag_off{0}, part_off{0};
    std::vector<uint32_t> part_rec;
    std::vector<uint8_t> part_mate;
    for (size_t t = 0; t < nt; ++t) {
        if (by_table[t])
            for (const PlannedFrag& pf : by_table[t]->plan.frags) {
                for (size_t k = 0; k < pf.parts.size(); ++k) { part_rec.push_back(slot_[pf.parts[k].rec] - 1); part_mate.push_back(pf.mate[k]); }
                part_off.push_back(part_rec.size());
            }
        frag_off.push_back(part_off.size() - 1);
    }
    if (part_rec.empty()) return;                                                          // no fragment with a cell in the whole round
    floria_fragment_plan plan{};
    plan.n_contigs = (uint32_t)nt; plan.frag_off = frag_off.data(); plan.part_off = part_off.data(); plan.part_rec = part_rec.data(); plan.set_order = nullptr;
    floria_assemble_options opts{};
    opts.flags = (derive_set_order ? FLORIA_ASM_DERIVE_SET_ORDER : 0u) | (keep_seq_pos ? FLORIA_ASM_KEEP_SEQ_POS : 0u);
    opts.part_mate = keep_seq_pos ? part_mate.data() : nullptr;
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    std::vector<floria_hip_contig*> raw(nt, nullptr);
    double t0 = now();
    if (const int rc = floria_hip_assemble_contigs_opt(s_.ctx(), summary_, &plan, &opts, raw.data()))
        throw Error(rc, std::string("floria_hip_assemble_contigs_opt: ") + floria_hip_last_error());
    std::vector<ContigHandle> handles(nt);
    for (size_t t = 0; t < nt; ++t) handles[t].reset(raw[t]);
    assemble_s += now() - t0;
    floria_timing tm;
    if (floria_hip_last_timing(s_.ctx(), &tm) == 0) assemble_ms += tm.total_ms;
    if (ignore_monomorphic) {                                                              // remove_monomorphic_allele (floria.rs:315-317) on the handles
        t0 = now();
        std::vector<uint64_t> snp_off{0};
        for (size_t t = 0; t < nt; ++t) snp_off.push_back(snp_off.back() + snp_count_[t]);
        std::vector<floria_hip_contig*> out(nt, nullptr);
        floria_mono_result* res = nullptr;
        if (const int rc = floria_hip_drop_monomorphic(s_.ctx(), raw.data(), (uint32_t)nt, snp_off.data(), epsilon, derive_set_order ? 1 : 0, out.data(), &res))
            throw Error(rc, std::string("floria_hip_drop_monomorphic: ") + floria_hip_last_error());
        for (size_t t = 0; t < nt; ++t) handles[t].reset(out[t]);                          // (frees the inputs)
        uint64_t reads_in = 0;
        for (size_t t = 0; t < nt; ++t) {
            HeaderContig* hc = by_table[t];
            const uint64_t off = res->read_off[t], n_new = res->read_off[t + 1] - off;
            if (!hc) continue;
            reads_in += hc->all_frags.size();
            std::vector<Frag> kept;
            kept.reserve(n_new);
            for (uint64_t r = 0; r < n_new; ++r) {                                         // drop, reorder, renumber; the survivors' ends come back with the map
                Frag& f = hc->all_frags[res->old_read[off + r]];
                f.first_position = res->new_first[off + r]; f.last_position = res->new_last[off + r]; f.counter_id = (size_t)r;
                kept.push_back(std::move(f));
            }
            hc->all_frags = std::move(kept);
        }
        removed_snps += res->n_removed_snps; dropped_reads += res->n_dropped_reads;
        bytes_back += 12 * reads_in + snp_off.back();
        floria_hip_mono_result_free(res);
        filter_s += now() - t0;
        if (floria_hip_last_timing(s_.ctx(), &tm) == 0) filter_ms += tm.total_ms;
    }
    for (size_t t = 0; t < nt; ++t) if (by_table[t]) by_table[t]->handle = std::move(handles[t]);
}

// --output-reads on a device segment: the sequences plan() keeps on a host segment — the base of every fragment and its second mate — in ONE call for the round
void ResidentPileup::fetch_sequences(std::vector<HeaderContig*>& planned) {
    if (!bam_.dev || !o_.output_reads) return;
    struct Dst { Frag* f; int mate; };
    std::vector<Dst> dst;
    std::vector<uint64_t> seq_off, qual_off;
    std::vector<uint32_t> l_seq;
    const auto want = [&](Frag& f, const PlannedFrag& pf) {
        for (size_t k = 0; k < pf.parts.size(); ++k) {
            if (k != 0 && !pf.mate[k]) continue;
            const BamRecord& rec = bam_.records[pf.parts[k].rec];
            dst.push_back({&f, k == 0 ? 0 : 1});
            seq_off.push_back((uint64_t)(uintptr_t)rec.seq.packed); qual_off.push_back((uint64_t)(uintptr_t)rec.qual.p); l_seq.push_back((uint32_t)rec.seq.n);
        }
    };
    for (HeaderContig* hc : planned) {
        if (!hc) continue;
        for (size_t k = 0; k < hc->all_frags.size(); ++k) want(hc->all_frags[k], hc->plan.frags[k]);
        for (size_t k = 0; k < hc->frags_without_snps.size(); ++k) want(hc->frags_without_snps[k], hc->plan.snpless[k]);
    }
    if (dst.empty()) return;
    const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    floria_blob_sequences* r = nullptr;
    if (const int rc = floria_hip_blob_sequences(s_.ctx(), bam_.dev->blob, seq_off.data(), l_seq.data(), qual_off.data(), dst.size(), &r))
        throw Error(rc, std::string("floria_hip_blob_sequences: ") + floria_hip_last_error());
    for (size_t i = 0; i < dst.size(); ++i) frag_sequences(*dst[i].f, dst[i].mate, r->bases + r->base_off[i], r->quals + r->base_off[i], (size_t)(r->base_off[i + 1] - r->base_off[i]));
    bytes_back += 2 * r->base_off[dst.size()] + 8 * (dst.size() + 1);
    floria_hip_blob_sequences_free(r);
    sequences_s += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
}

BamFile host_copy_of_target(const BamFile& seg, const std::string& contig, size_t threads) {
    BamFile out;
    out.target_names = seg.target_names; out.target_len = seg.target_len;
    out.by_tid.resize(seg.target_names.size());
    out.tid_begin = seg.tid_begin; out.tid_end = seg.tid_end;
    const auto tid_it = std::find(seg.target_names.begin(), seg.target_names.end(), contig);
    if (!seg.dev || tid_it == seg.target_names.end()) return out;
    const std::vector<uint32_t>& recs = seg.by_tid[(size_t)(tid_it - seg.target_names.begin())];
    if (recs.empty()) return out;
    // (a target's records are neighbours in the blob: one chain, or one stretch of the segment's only chain)
    const DeviceSegment& d = *seg.dev;
    const uint64_t lo = d.rec_off[recs.front()], hi = d.rec_end[recs.back()];
    out.raw.resize((size_t)(hi - lo));
    if (const int rc = floria_hip_blob_download(d.blob, lo, out.raw.data(), hi - lo)) throw Error(rc, std::string("floria_hip_blob_download: ") + floria_hip_last_error());
    d.bytes_down += hi - lo;
    decode_records(out, 0, out.raw.size(), "the records of contig " + contig, threads);
    return out;
}

std::pair<std::vector<Frag>, std::vector<Frag>> get_frags_from_bamvcf_rewrite(const BamFile& bam, const VcfProfile& vp, const Options& o, const std::string& contig,
                                                                               const std::string* ref_seq) {
    return ContigIngest(bam, vp, o, contig, ref_seq, nullptr).finish();
}

void RealignQueue::append(RealignQueue&& o) {
    read_windows.insert(read_windows.end(), o.read_windows.begin(), o.read_windows.end());
    ref_windows.insert(ref_windows.end(), o.ref_windows.begin(), o.ref_windows.end());
    alleles.insert(alleles.end(), o.alleles.begin(), o.alleles.end());
    n_alleles.insert(n_alleles.end(), o.n_alleles.begin(), o.n_alleles.end());
    dst.insert(dst.end(), o.dst.begin(), o.dst.end());
    o = RealignQueue();
}

// file_reader.rs:749-826.  The htslib pileup engine visits every reference position covered by at least one alignment that
// passes its default mask (unmapped | secondary | qc-fail | duplicate are dropped), contig by contig in coordinate order.
struct EpsilonEstimator::Impl {
    size_t count = 0;
    std::vector<double> err_vec;                           // one per sampled column with total >= 5: n_err is its size
    std::map<size_t, uint64_t> lengths;                    // the multiset of the read lengths: l_seq -> multiplicity
    std::vector<std::array<int64_t, 4>> columns;           // every sampled column: tid, pos, total, most (--dump-estimate)
    bool done = false;
    static constexpr size_t stop = 1000;
};
EpsilonEstimator::EpsilonEstimator() : p_(new Impl) {}
EpsilonEstimator::~EpsilonEstimator() = default;
bool EpsilonEstimator::done() const { return p_->done; }
void EpsilonEstimator::add_length(size_t l_seq, uint64_t hits) { if (hits) p_->lengths[l_seq] += hits; }
void EpsilonEstimator::add_column(int32_t tid, int32_t pos, uint32_t total, uint32_t most) {
    p_->columns.push_back({tid, pos, total, most});
    if (total >= 5) p_->err_vec.push_back(((double)total - (double)most) / (double)most);
}
void EpsilonEstimator::feed(const BamFile& bam) {
    size_t& count = p_->count;
    std::vector<double>& err_vec = p_->err_vec;
    bool& done = p_->done;
    if (done) return;
    struct Aln { const BamRecord* r; int64_t beg, end; };
    std::vector<std::vector<Aln>> by_tid(bam.target_names.size());
    for (const BamRecord& r : bam.records) {
        if (r.tid < 0 || (size_t)r.tid >= by_tid.size() || (r.flags & F_ERRORS) || r.cigar.empty()) continue;
        by_tid[r.tid].push_back({&r, r.pos, reference_end(r)});
    }
    const size_t stop = Impl::stop;
    auto base_at = [](const BamRecord& r, int64_t pos, char* base) -> bool {          // false: deletion / refskip / not aligned here
        size_t q = 0; int64_t ref = r.pos;
        for (size_t ck = 0; ck < r.cigar.size(); ++ck) {
            const uint32_t c = r.cigar[ck];
            const int op = cig_op(c); const int64_t len = cig_len(c);
            if (consumes_r(op) && pos < ref + len) {
                if (!(op == 0 || op == 7 || op == 8)) return false;
                const size_t sp = q + (size_t)(pos - ref);
                if (sp >= r.seq.size()) return false;
                *base = r.seq[sp];
                return true;
            }
            if (consumes_q(op)) q += (size_t)len;
            if (consumes_r(op)) ref += len;
        }
        return false;
    };
    for (size_t tid = 0; tid < by_tid.size(); ++tid) {
        std::vector<Aln>& alns = by_tid[tid];
        if (done) break;
        std::stable_sort(alns.begin(), alns.end(), [](const Aln& a, const Aln& b) { return a.beg < b.beg; });
        size_t next = 0;
        std::vector<Aln> active;
        int64_t pos = 0;
        while (!done && (next < alns.size() || !active.empty())) {
            if (active.empty()) pos = std::max(pos, alns[next].beg);
            while (next < alns.size() && alns[next].beg <= pos) active.push_back(alns[next++]);
            active.erase(std::remove_if(active.begin(), active.end(), [&](const Aln& a) { return a.end <= pos; }), active.end());
            if (active.empty()) continue;
            // a pileup column at `pos`
            if (count % 1000 != 0) {
                // skip ahead: columns are consecutive while the active set is non-empty; stop where the set can change
                int64_t lim = INT64_MAX;
                for (const Aln& a : active) lim = std::min(lim, a.end);
                if (next < alns.size()) lim = std::min(lim, alns[next].beg);
                const int64_t cols = std::max<int64_t>(1, lim - pos);
                const int64_t to_sample = 1000 - (int64_t)(count % 1000);
                const int64_t step = std::min(cols, to_sample);
                count += (size_t)step; pos += step;
                continue;
            }
            uint32_t most_base = 0, total_c = 0;
            uint32_t base_cnt[256] = {0};
            for (const Aln& a : active) {
                char b;
                if (!base_at(*a.r, pos, &b)) continue;
                if ((a.r->flags & F_ERRORS) || (a.r->flags & F_SECONDARY) || a.r->seq.empty()) continue;
                add_length(a.r->seq.size(), 1);
                base_cnt[(unsigned char)b] += 1;
            }
            for (uint32_t v : base_cnt) { if (v > most_base) most_base = v; total_c += v; }
            add_column((int32_t)tid, (int32_t)pos, total_c, most_base);
            ++pos;
            if (total_c < 5) continue;                                       // (count is not advanced: the next column is sampled too)
            if (err_vec.size() >= stop && !p_->lengths.empty()) { done = true; break; }
            ++count;
        }
    }
}
void EpsilonEstimator::feed_device(const BamFile& bam) {
    if (p_->done) return;
    if (!bam.dev || !bam.dev->blob) throw Error(FLORIA_E_INVALID, "EpsilonEstimator::feed_device: not a device segment");
    // the three filters on the table's fields, the records of every target in position order (the order the host pass sorts them into)
    std::vector<int32_t> pos;
    std::vector<uint64_t> cigar_off, seq_off, group_off{0};
    std::vector<uint32_t> n_cigar, l_seq;
    std::vector<int32_t> group_tid;
    for (size_t tid = 0; tid < bam.by_tid.size(); ++tid) {
        std::vector<uint32_t> ix;
        for (const uint32_t i : bam.by_tid[tid]) { const BamRecord& r = bam.records[i]; if (!(r.flags & F_ERRORS) && !r.cigar.empty()) ix.push_back(i); }
        if (ix.empty()) continue;
        std::stable_sort(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return bam.records[a].pos < bam.records[b].pos; });
        for (const uint32_t i : ix) {
            const BamRecord& r = bam.records[i];
            pos.push_back((int32_t)r.pos); cigar_off.push_back((uint64_t)(uintptr_t)r.cigar.p); n_cigar.push_back((uint32_t)r.cigar.n);
            seq_off.push_back((uint64_t)(uintptr_t)r.seq.packed); l_seq.push_back((uint32_t)r.seq.n);
        }
        group_off.push_back(pos.size()); group_tid.push_back((int32_t)tid);
    }
    floria_estimate_records recs{};
    recs.n = pos.size(); recs.pos = pos.data(); recs.cigar_off = cigar_off.data(); recs.n_cigar = n_cigar.data(); recs.seq_off = seq_off.data(); recs.l_seq = l_seq.data();
    recs.n_groups = (uint32_t)group_tid.size(); recs.group_off = group_off.data();
    floria_estimate_state st{p_->count, (uint32_t)p_->err_vec.size()};
    floria_estimate_result* res = nullptr;
    if (const int rc = floria_hip_blob_estimate(bam.dev->ctx, bam.dev->blob, &recs, (uint32_t)Impl::stop, &st, &res)) throw Error(rc, std::string("floria_hip_blob_estimate: ") + floria_hip_last_error());
    for (uint64_t c = 0; c < res->n_cols; ++c) add_column(group_tid[res->col_group[c]], res->col_pos[c], res->col_total[c], res->col_most[c]);
    for (size_t i = 0; i < pos.size(); ++i) add_length(l_seq[i], res->rec_hits[i]);
    p_->count = (size_t)st.count;
    p_->done = res->done != 0;
    floria_hip_estimate_result_free(res);
    if (p_->err_vec.size() != st.n_err) throw Error(FLORIA_E_DEVICE, "floria_hip_blob_estimate: the columns returned do not add up to the state returned");
    floria_timing tm{};
    if (floria_hip_last_timing(bam.dev->ctx, &tm) == 0) { device_kernel_ms += tm.pileup_ms; device_h2d_ms += tm.h2d_ms; device_d2h_ms += tm.d2h_ms; }
    ++device_calls;
}
void EpsilonEstimator::dump(std::ostream& out) const {
    for (const auto& c : p_->columns) out << c[0] << " " << c[1] << " " << c[2] << " " << c[3] << "\n";
    out << "count " << p_->count << "\nn_err " << p_->err_vec.size() << "\n";
    for (const auto& kv : p_->lengths) out << "length " << kv.first << " " << kv.second << "\n";
}
std::pair<size_t, double> EpsilonEstimator::result() {
    std::vector<double>& err_vec = p_->err_vec;
    uint64_t n = 0;
    for (const auto& kv : p_->lengths) n += kv.second;
    if (n == 0) return {500, 0.01};
    uint64_t at = n * 66 / 100;                                              // read_lengths[len * 66 / 100] of the sorted multiset
    size_t q_66 = 0;
    for (const auto& kv : p_->lengths) { if (at < kv.second) { q_66 = kv.first; break; } at -= kv.second; }
    std::sort(err_vec.begin(), err_vec.end());
    const double med66 = err_vec.empty() ? 0.0 : err_vec[err_vec.size() * 66 / 100];
    return {std::max<size_t>(q_66, 500), std::max(med66, 0.01)};             // constants::MINIMUM_BLOCK_SIZE = 500
}

std::pair<size_t, double> l_epsilon_auto_detect(const BamFile& bam) {
    EpsilonEstimator e;
    e.feed(bam);
    return e.result();
}

}  // namespace floria
