// floria-hip — command-line driver with the reference's flags (floria.rs:21-196, parse_cmd_line.rs:11-196) and its per-contig
// flow (floria.rs:229-388): ingest -> generate_hap_graph (device) -> solve_lp_graph -> get_disjoint_paths_rewrite ->
// process_reads_for_final_parts (device) -> get_frags_in_snpless_gaps -> write_outputs.  The contigs take that flow in BATCHES:
// the host stages of a batch run one contig per task on -t threads, every device stage runs once per batch (a metagenome is
// thousands of small contigs; one device call per contig and stage would be launch-latency-bound).  Files are those of the
// per-contig flow, byte for byte.
//
//   floria-hip -b reads.bam -v calls.vcf -r reference.fa -o results [-e 0.04] [-l 10000] [-n 10] [-p 5] [-d 0.0005] [-s 2] [-m 15]
//              [-t 10] [-G contig ...] [-X] [--no-stop-heuristic] [--snp-count-filter 100] [--supp-aln-dist-cutoff 40000] [--overwrite]
//
//              [--output-reads [--gzip-reads] [--extra-trimming]] [--ignore-monomorphic]
// Flags of the reference that are not supported and say so: the hidden -H/--hybrid, --reassign-short, --bin-by-cov (-q is accepted and
// ignored, as in the reference).  Extras: --device N, --devices LIST (e.g. 0-7 or 0,2,5: the contigs of a batch are dealt to these GPUs of the node,
// longest first; one context and one host thread per device; the files are those of a one-GPU run),
// --batch-contigs N / --batch-cells N (size of a device batch), --debug (debug_graph.txt per contig), --lp-tie first|last (which optimal vertex of the
// stitching LP is used where the optimum is not unique; the run reports how many contigs that concerns), and for tests --dump-frags FILE,
// --dump-seq-pos FILE, --ingest-only, --no-realign, --stitch-graph FILE.
// --pileup host | device: where the CIGAR walk that turns alignment records into SNP calls runs.  host [default]: frag_from_record on -t threads, one contig per task;
// device: one floria_hip_pileup_records call per ingest round for every record that passes the alignment filter, the Frags filled from its cells (same files).
// fused: device, with the realignment of the calls done by the same call (floria_hip_pileup_records_realign) before the cells come back; without realignment (--no-realign)
// it is device.  Same files.
// resident: one floria_hip_pileup_records_resident call per ingest round (re-aligned there unless --no-realign); the cells stay on the device.  Per contig a fragment plan
// is made from names, flags and the per-record spans of the call's summary (combine_frags on headers, ingest.cpp: plan_contig), one floria_hip_assemble_contigs_opt call turns
// the round's plans into resident contigs, --ignore-monomorphic is one floria_hip_drop_monomorphic call on them; the batch phases on the handles, the writers take their
// allele tables from floria_hip_haploset_alleles and --output-reads' trims from floria_hip_read_spans.  A contig the device cannot number (see --pileup device) keeps the host
// walk and is uploaded beside the others.  One device only, no --dump-frags (the qualities are folded into weights on the device).  Same files.
// --haplosets host | resident: where the haplosets live between S2 and the writers, on any --pileup route.  host [default]: floria_hip_reassign_batch returns the group
// lists and COV / ERR, HAPQ, the allele tables and the read trims take them up again.  resident: floria_hip_reassign_batch_resident splits and sorts on the device and
// keeps the haplosets there as a handle; the lists come back once (floria_hip_haplosets_download) for the writers and the four calls take the handle (the allele tables and
// trims of a batch that mixes contigs with and without a handle of their own still go by lists).  Same files.
// For tests: --dump-plan FILE (with --ingest-only, any route: the fragment plan per contig), --dump-estimate FILE (with --ingest-only, either --estimate route: the sampled columns and the state of the -e / -l
// estimate), --dump-handles FILE (any route: the resident arrays of every contig of every batch).
// --inflate host | device (with --pileup resident): where the BGZF members are inflated.  host [default]: on the host threads, the inflated records uploaded for the walk.
// device: BamStream plans runs of adjacent members from their headers (inflate_on_device), floria_hip_inflate_bgzf inflates them into a blob, floria_hip_blob_records_opt
// returns the header-sized record table, the walk reads the blob (floria_hip_pileup_records_resident_blob); a CG-tag record's and a host-walk contig's bytes come down by
// floria_hip_blob_download, --output-reads' sequences by one floria_hip_blob_sequences call per ingest round.  The header and the -e / -l estimate stay on the host
// (the estimate unless --estimate device: its pass then reads device segments of the stream in file order and one floria_hip_blob_estimate call per segment).  The next
// segment's inflate does NOT overlap the current batch's phasing (not built).  The log gains one line.  Same files.
// --no-index: a .bai beside the BAM (X.bam.bai, then X.bai) is used when present - the contigs that -G and --snp-count-filter leave are read through it, each from its
// indexed offset, and the log gains one line (contigs selected, BGZF members inflated, members in the file); --no-index streams the whole file in order as without one.  Same files.
// --realign exact | block:STEP,RULE,TIE: how the windows around SNP calls are scored.  exact [default]: the exact affine-gap DP; block:STEP,RULE,TIE (STEP 1 | 2 | 4 | 8,
// RULE max | sum, TIE right | down): one member of the family of fixed-block walks (block 8) that scripts/probes/block_walk.c defines.  The reference's block-aligner is
// some heuristic of this kind; which member, if any, is not known, so there is no bare `block`.  The run's log and cmd.log name the scoring used.
#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>

#include "cli.hpp"
#include "floria_host.hpp"

using namespace floria;

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

// one task per index on up to `threads` std::threads; the first exception is rethrown on the caller
template <class F> static void parallel_for(size_t n, size_t threads, F&& f) {
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

// hap graph, flows and paths of a contig in the N / E / F / P line format (--debug; tests/test_gpu_cli.py reads it back)
static void write_debug_graph(const ContigWork& w) {
    struct stat st;
    if (stat(w.out_dir.c_str(), &st) != 0) mkdir(w.out_dir.c_str(), 0777);
    std::ofstream g(w.out_dir + "/debug_graph.txt", std::ios::trunc);
    g.precision(17);
    for (const auto& col : w.hap_graph) for (const HapNode& n : col) {
        g << "N\t" << n.column << "\t" << n.row << "\t" << n.id << "\t" << n.cov << "\t" << n.snp_endpoints.first << "\t" << n.snp_endpoints.second;
        for (const Frag* f : n.frag_set) g << "\t" << f->counter_id;
        g << "\n";
    }
    for (const auto& col : w.hap_graph) for (const HapNode& n : col) for (const auto& e : n.out_edges) g << "E\t" << n.column << "\t" << n.row << "\t" << e.first << "\t" << e.second << "\n";
    for (const FlowUpdate& f : w.flows) g << "F\t" << f.n1.first << "\t" << f.n1.second << "\t" << f.n2.second << "\t" << f.flow << "\n";
    for (size_t k = 0; k < w.path_parts.size(); ++k) {
        g << "P\t" << w.path_ranges[k].first << "\t" << w.path_ranges[k].second;
        for (const Frag* f : w.path_parts[k]) g << "\t" << f->counter_id;
        g << "\n";
    }
}

namespace {

const char* scoring_name(const Options& o, std::string& buf) { return o.realign_walk ? (buf = "fixed-block walk " + realign_spec(o)).c_str() : "exact affine-gap DP"; }

// Every run-total timer and counter of the driver, the notices that are given once per run, and the closing lines made of them
struct RunStats {
    const double t_all = now_s();
    double t_ingest = 0., t_s1 = 0., t_stitch = 0., t_s2 = 0., t_stats = 0., t_write = 0., t_realign = 0., t_stream = 0.;
    size_t n_realign_device = 0, n_batches = 0, n_records = 0, n_segments = 0;
    size_t n_pileup_records = 0, n_pileup_bytes = 0, n_pileup_calls = 0;      // --pileup device
    double t_pileup = 0., t_pileup_kernels = 0., t_pileup_h2d = 0., t_pileup_d2h = 0.;
    floria_realign_counts fused_counts = {};
    bool said_host_walk = false;
    bool warn_first_length = true;
    // The reference-arithmetic mode adds a read's terms in the iteration order of its position set.  For a fragment built from ONE alignment the library emulates that
    // set on the device (arith_kernel.h); fragments whose set was EXTENDED by a mate or a supplementary piece (file_reader.rs:541, 639) or cut down by
    // --ignore-monomorphic (utils_frags.rs:745-755) carry what their set went through (Frag::position_segments / removed_positions, ingest.cpp) and a Batch hands
    // the replayed order to the library (floria_pileup_packed::set_order): round 6; until then such batches fell back to the canonical form under --arith auto.
    size_t n_batches_orders = 0, n_frags_merged = 0, n_frags_cut = 0;
    size_t n_resident_merged = 0, n_resident_contigs = 0;
    double t_resident_assemble = 0., t_resident_filter = 0., t_resident_assemble_ev = 0., t_resident_filter_ev = 0.;
    std::atomic<uint64_t> n_haplosets_by_handle{0};                          // --haplosets resident
    std::atomic<uint64_t> n_paths_joined{0};                                 // --paths resident
    uint64_t resident_bytes_back = 0, resident_removed_snps = 0, resident_dropped_reads = 0;
    uint64_t inflate_host_walk_bytes = 0;                                    // --inflate device: record bytes that came down for contigs that keep the host walk
    double t_blob_sequences = 0.;                                            // ... and the seconds of the rounds' floria_hip_blob_sequences calls
    // --estimate device: the segments the estimate's pass read (they are inside the stream's totals), its wall seconds and the device events of its calls
    size_t estimate_segments = 0, estimate_calls = 0;
    double t_estimate = 0., t_estimate_kernels = 0., t_estimate_h2d = 0., t_estimate_d2h = 0.;
    std::atomic<size_t> lp_contigs{0}, lp_not_unique{0}, lp_edges{0}, lp_movable{0};

    // a round's device walk, whichever route made it; says once which contig keeps the host walk
    void add_walk(const RoundWalk& w, double wall_s, PileupRoute route) {
        t_pileup += wall_s;
        fused_counts.cells += w.counts.cells; fused_counts.in_bounds += w.counts.in_bounds; fused_counts.shortcut += w.counts.shortcut;
        fused_counts.scored += w.counts.scored; fused_counts.changed += w.counts.changed;
        ++n_pileup_calls; n_pileup_records += w.records_sent; n_pileup_bytes += w.blob_bytes;
        t_pileup_kernels += w.kernel_ms * 1e-3; t_pileup_h2d += w.h2d_ms * 1e-3; t_pileup_d2h += w.d2h_ms * 1e-3;
        if (!w.host_contigs.empty() && !said_host_walk) {
            said_host_walk = true;
            fprintf(stderr, "floria-hip: --pileup %s: contig %s keeps the host walk (its SNP numbers are not their rank in position order, or a site has more than %d alleles)%s; "
                            "this is said once\n", route_name(route), w.host_contigs[0].c_str(), FLORIA_MAX_ALLELES,
                    route == PileupRoute::Resident ? " and is uploaded beside the resident contigs of its batch" : "");
        }
    }
    // a round's assemble (and filter) call
    void add_assembly(const ResidentPileup& r) {
        t_resident_assemble += r.assemble_s; t_resident_filter += r.filter_s;
        t_resident_assemble_ev += r.assemble_ms * 1e-3; t_resident_filter_ev += r.filter_ms * 1e-3;
        resident_bytes_back += r.bytes_back; resident_removed_snps += r.removed_snps; resident_dropped_reads += r.dropped_reads;
        t_blob_sequences += r.sequences_s;
    }
    // a batch under the reference arithmetic: the fragments whose set order is replayed on the host
    void add_set_orders(const std::vector<ContigWork>& work) {
        size_t merged = 0, cut = 0;
        for (const ContigWork& w : work) if (!w.handle) for (const Frag& f : w.all_frags) { merged += f.merged_positions ? 1 : 0; cut += f.removed_positions.empty() ? 0 : 1; }
        n_frags_merged += merged; n_frags_cut += cut;
        if (merged || cut) ++n_batches_orders;
    }
    void report(const Cli& cli, const BamStream& stream, bool reference_arith) const {
        const Options& o = cli.o;
        std::string buf;
        fprintf(stderr, "BAM: %zu records in %zu segments, %.3fs of inflate + decode, largest inflated buffer %zu MiB\n", n_records, n_segments, t_stream, stream.peak_buffer_bytes() >> 20);
        if (!stream.index_path().empty()) {
            const BamStream::IndexUse u = stream.index_use();
            fprintf(stderr, "BAM index %s: %zu targets selected, %zu BGZF members inflated for them of %zu in the file\n", stream.index_path().c_str(), u.selected, u.members_inflated,
                    u.members_in_file);
        }
        const bool behind_walk = realigned_behind_walk(o.pileup, cli.no_realign);
        if (!behind_walk || n_realign_device)                                     // (fused, resident: only the contigs that kept the host walk queue windows)
        fprintf(stderr, "Realignment: %zu calls scored on the device in %.3fs (inside the ingest time), scoring %s\n", n_realign_device, t_realign, scoring_name(o, buf));
        if (behind_walk)
            fprintf(stderr, "Realignment: %llu calls scored on the device behind the walk (%llu by the exact shortcut, %llu outside the window bounds), scoring %s\n",
                    (unsigned long long)fused_counts.scored, (unsigned long long)fused_counts.shortcut, (unsigned long long)(fused_counts.cells - fused_counts.in_bounds),
                    scoring_name(o, buf));
        if (walk_on_device(o.pileup))
            fprintf(stderr, "Pileup on the device: %zu records, %zu blob bytes in %zu calls, %.3fs (inside the ingest time; device events: upload %.3fs, kernels %.3fs, download %.3fs)\n",
                    n_pileup_records, n_pileup_bytes, n_pileup_calls, t_pileup, t_pileup_h2d, t_pileup_kernels, t_pileup_d2h);
        if (o.pileup == PileupRoute::Resident) {
            fprintf(stderr, "Resident contigs: %zu assembled on the device in %.3fs (device events %.3fs), --ignore-monomorphic filter %.3fs (device events %.3fs; %llu SNPs removed, %llu reads dropped); "
                            "%llu bytes came back (record summaries, filter maps, allele tables, read trims), no cell\n", n_resident_contigs, t_resident_assemble, t_resident_assemble_ev,
                    t_resident_filter, t_resident_filter_ev, (unsigned long long)resident_removed_snps, (unsigned long long)resident_dropped_reads, (unsigned long long)resident_bytes_back);
            if (reference_arith)
                fprintf(stderr, "Arithmetic: the set orders of %zu fragments merged from several alignments were derived on the device (floria_hip_assemble_contigs_opt), every resident contig "
                                "phased in the reference's running sums\n", n_resident_merged);
        }
        if (cli.inflate_device) {
            const BamStream::DeviceUse u = stream.device_use();
            fprintf(stderr, "Inflate on the device: %zu segments, %zu BGZF members sent (%llu compressed bytes up, %llu inflated bytes on the device), %zu segments re-planned for look-ahead, "
                            "%zu members re-inflated as carry-over, %llu bytes down for host use (%llu for host-walk contigs, %llu for CG records); inflate %.3fs, record table %.3fs, "
                            "sequences %.3fs\n", u.segments, u.members, (unsigned long long)u.compressed_bytes, (unsigned long long)u.inflated_bytes, u.replanned, u.carried_members,
                    (unsigned long long)(inflate_host_walk_bytes + u.cg_bytes_down), (unsigned long long)inflate_host_walk_bytes, (unsigned long long)u.cg_bytes_down, u.inflate_s, u.table_s,
                    t_blob_sequences);
            if (estimate_calls)
                fprintf(stderr, "Estimate on the device: %zu of those segments read by the -e / -l estimate in %.3fs (%zu floria_hip_blob_estimate calls; device events: upload %.3fs, "
                                "kernels %.3fs, download %.3fs)\n", estimate_segments, t_estimate, estimate_calls, t_estimate_h2d, t_estimate_kernels, t_estimate_d2h);
        }
        if (o.haplosets_resident)
            fprintf(stderr, "Haplosets: %llu split, sorted and kept on the device behind S2 (floria_hip_reassign_batch_resident); one download for the writers, COV / ERR, HAPQ, "
                            "allele tables and read trims by handle\n", (unsigned long long)n_haplosets_by_handle.load());
        if (o.paths_resident)
            fprintf(stderr, "Paths: --paths resident: %llu hap-graph paths joined into haplosets on the device (floria_hip_join_paths), S2 from that handle "
                            "(floria_hip_reassign_haplosets_resident); S1 %s\n", (unsigned long long)n_paths_joined.load(),
                    o.paths_keep_lists ? "returned its read lists (--debug prints them)" : "returned no read list");
        fprintf(stderr, "Batches %zu; ingest %.3fs, phasing (upload + S1 + graph) %.3fs, LP + paths %.3fs, S2 %.3fs, COV/ERR/HAPQ %.3fs, writers %.3fs\n", n_batches, t_ingest, t_s1,
                t_stitch, t_s2, t_stats, t_write);
        if (reference_arith && n_batches_orders)
            fprintf(stderr, "Arithmetic: %zu of %zu batches carried the set orders of fragments that are not one alignment's (%zu merged from several alignments, %zu cut down by "
                            "--ignore-monomorphic): replayed on the host, every batch phased in the reference's running sums\n", n_batches_orders, n_batches, n_frags_merged, n_frags_cut);
        if (cli.lp_report)
        fprintf(stderr, "LP: the optimum is not unique for %zu of %zu contigs (%zu of %zu edge flows differ in some other optimal solution); this run used the '%s' vertex, "
                        "rerun with --lp-tie %s to see what depends on it\n", lp_not_unique.load(), lp_contigs.load(), lp_movable.load(), lp_edges.load(),
                cli.lp_tie == LpTie::First ? "first" : "last", cli.lp_tie == LpTie::First ? "last" : "first");
        fprintf(stderr, "Total time taken is %.3fs\n", now_s() - t_all);
    }
};

// What the steps of a run share: the command line, the inputs read once, the contexts, and the dump files of the tests
struct Run {
    const Cli& cli;
    const VcfProfile& vp;
    const std::map<std::string, std::string>& fasta;
    const std::vector<std::string>& contigs;                                  // get_contigs_to_phase (file_reader.rs:738-746)
    const std::vector<std::unique_ptr<Session>>& sessions;
    const bool reference_arith;
    const size_t n_threads;
    std::ofstream dump, dump_sp, dump_pl, dump_hd;
    std::mutex dump_hd_mu;
    Session& walker() const { return *sessions[0]; }                         // the context of the device walks and of the realignment queue
    Run(const Cli& c, const VcfProfile& v, const std::map<std::string, std::string>& f, const std::vector<std::string>& names, const std::vector<std::unique_ptr<Session>>& s, bool ref_arith)
        : cli(c), vp(v), fasta(f), contigs(names), sessions(s), reference_arith(ref_arith), n_threads(std::max<size_t>(1, c.o.num_threads)) {
        if (!cli.dump_frags.empty()) dump.open(cli.dump_frags, std::ios::trunc);
        if (!cli.dump_seq_pos.empty()) dump_sp.open(cli.dump_seq_pos, std::ios::trunc);
        if (!cli.dump_plan.empty()) dump_pl.open(cli.dump_plan, std::ios::trunc);
        if (!cli.dump_handles.empty()) dump_hd.open(cli.dump_handles, std::ios::trunc);
    }
    void close_dumps() {
        if (dump.is_open()) dump.close();
        if (dump_sp.is_open()) dump_sp.close();
        if (dump_pl.is_open()) dump_pl.close();
        if (dump_hd.is_open()) dump_hd.close();
    }
    bool listed(const std::string& contig) const {                           // -G
        const std::vector<std::string>& l = cli.o.list_to_phase;
        return l.empty() || std::find(l.begin(), l.end(), contig) != l.end();
    }
    bool enough_snps(const std::string& contig) const {                      // --snp-count-filter
        const auto pam = vp.vcf_pos_allele_map.find(contig);
        return pam != vp.vcf_pos_allele_map.end() && pam->second.size() >= cli.o.snp_count_filter;
    }
};

struct Arithmetic { bool reference_arith; std::string run_note; };           // run_note: second line of cmd.log

// ---- the epsilon policy (DESIGN.md "Arithmetic").  Every weighted sum of the phasing path is an exact multiple of 2^-24; the only inexact
// terms of the reference are its running `+= epsilon` additions, whose rounding depends on hash-map iteration order unless epsilon is dyadic.
// For an epsilon that is a multiple of 2^-10 every one of those sums is exact in f64 in ANY order, so the function this library computes IS the
// reference's function.  An auto-estimated epsilon (parse_cmd_line.rs:72-90) is used AS ESTIMATED, like the reference does, and cmd.log has the
// reference's single line; --epsilon-round rounds it to the nearest multiple of 2^-10 (a change of at most 0.0005 to a coverage-sampled average)
// and records both values on a second line of cmd.log.  Whatever its origin, an epsilon that is not such a multiple gets one warning on stderr:
// results are then an equally good solution, but may differ from the Rust binary's where scores tie in exact arithmetic.
// Fills o.block_length / o.epsilon where they were not given (the seconds of that first pass go to t_bam).
// `estimate_ctx` (--estimate device): the pass reads device segments - file order from the first record on, complete targets, as the host pass does - and the
// stream is rewound behind it as behind the host pass.
Arithmetic epsilon_policy(Cli& cli, BamStream& stream, double& t_bam, floria_hip_ctx* estimate_ctx, RunStats& stats) {
    Options& o = cli.o;
    std::string run_note;
    auto dyadic10 = [](double e) { const double k = e * 1024.0; return k == std::floor(k); };
    if (!cli.have_e || !cli.have_l) {                                             // parse_cmd_line.rs:72-90
        const double tp = now_s();
        EpsilonEstimator estimator;                                               // (a first pass over as much of the file as 1000 sampled columns need)
        if (estimate_ctx) {
            stream.inflate_on_device(estimate_ctx);
            BamFile seg;
            while (!estimator.done() && stream.next(seg, cli.bam_window)) { estimator.feed_device(seg); ++stats.estimate_segments; }
            stats.estimate_calls = estimator.device_calls;
            stats.t_estimate_kernels = estimator.device_kernel_ms * 1e-3; stats.t_estimate_h2d = estimator.device_h2d_ms * 1e-3; stats.t_estimate_d2h = estimator.device_d2h_ms * 1e-3;
        } else {
            BamFile seg;
            while (!estimator.done() && stream.next(seg, cli.bam_window)) estimator.feed(seg);
        }
        stream.rewind();
        const auto est = estimator.result();
        stats.t_estimate = now_s() - tp;
        t_bam += now_s() - tp;
        if (!cli.dump_estimate.empty()) {
            std::ofstream out(cli.dump_estimate, std::ios::trunc);
            if (!out) throw Error(FLORIA_E_INVALID, "cannot write " + cli.dump_estimate);
            estimator.dump(out);
        }
        if (!cli.have_l) o.block_length = est.first;
        if (!cli.have_e) {
            o.epsilon = est.second;
            if (cli.eps_round) {
                o.epsilon = std::max(1.0, std::floor(est.second * 1024.0 + 0.5)) / 1024.0;
                char buf[256];
                snprintf(buf, sizeof buf, "# floria-hip: -e estimated %.17g, used %.10g (rounded to a multiple of 2^-10: every sum of the phasing path is then exact in f64; "
                                          "requested by --epsilon-round)", est.second, o.epsilon);
                run_note = buf;
            }
        }
        fprintf(stderr, "Estimated -l %zu, -e %g (used where not given: -l %zu, -e %.10g)\n", est.first, est.second, o.block_length, o.epsilon);
    }
    const bool reference_arith = cli.arith_opt == "reference" || (cli.arith_opt == "auto" && !dyadic10(o.epsilon));
    if (!dyadic10(o.epsilon)) {
        const double near = std::max(1.0, std::floor(o.epsilon * 1024.0 + 0.5)) / 1024.0;
        if (reference_arith)
            fprintf(stderr, "floria-hip: note: -e %.17g is not a multiple of 2^-10: phasing in floria's own running-sum arithmetic (sums of epsilon terms rounded term by term, in the "
                            "iteration order of its hash containers; slower kernels).  --arith canonical keeps the fast kernels (every sum rounded once), -e %.10g is an epsilon at which "
                            "the two are the same function\n", o.epsilon, near);
        else
            fprintf(stderr, "floria-hip: warning: -e %.17g is not a multiple of 2^-10; with --arith canonical sums of epsilon terms are rounded once here and term by term (in hash-map order) in floria, "
                            "so haplosets can differ from floria's in exact ties (-e %.10g, or --epsilon-round for an estimated one, avoids that)\n", o.epsilon, near);
    }
    if (o.realign_walk) {
        if (!run_note.empty()) run_note += "\n";
        run_note += "# floria-hip: realignment scored by the fixed-block walk " + realign_spec(o) + " (block 8; default: the exact affine-gap DP)";
    }
    return {reference_arith, run_note};
}

// one context per device of --devices (default: the one --device); every one throws without a usable MI355X: no CPU fallback
std::vector<std::unique_ptr<Session>> open_sessions(const Cli& cli) {
    std::vector<int> devices = cli.devices;
    if (devices.empty()) devices.push_back(cli.o.device);
    std::vector<std::unique_ptr<Session>> sessions;
    if (needs_session(cli.o.pileup, cli.ingest_only)) for (int d : devices) sessions.emplace_back(new Session(d));     // (--ingest-only --pileup device | resident needs a device for the walk)
    return sessions;
}

// every contig that will be phased must be in the reference FASTA: said before anything is written, not when its batch comes up
void check_contigs_in_fasta(const Run& run) {
    for (const std::string& contig : run.contigs) {
        if (!run.listed(contig) || !run.enough_snps(contig)) continue;
        if (run.fasta.find(contig) == run.fasta.end()) throw Error(FLORIA_E_INVALID, "contig " + contig + " is not in the reference fasta");
    }
}

// ---- which contigs (floria.rs:229-262): those of the segment that -G names and that have enough SNPs
std::vector<std::string> contigs_of_segment(const Run& run, RunStats& stats, const BamFile& bam) {
    std::vector<std::string> todo;
    for (int32_t tid = bam.tid_begin; tid < bam.tid_end; ++tid) {
        const std::string& contig = run.contigs[(size_t)tid];
        if (!run.listed(contig)) continue;
        if (!run.enough_snps(contig)) {
            if (stats.warn_first_length)
                fprintf(stderr, "A contig (%s) is not present or has < %zu variants. This warning will not be shown from now on. Make sure to change --snp-count-filter if you want to phase small contigs.\n",
                        contig.c_str(), run.cli.o.snp_count_filter);
            stats.warn_first_length = false;
            continue;
        }
        todo.push_back(contig);
    }
    return todo;
}

// One ingest round, the contigs names[0 .. take) of the segment: records -> Frags with the realignment's undecided windows queued (one queue per contig), the
// queued windows of the whole round scored by ONE device call, then the merge of mates / supplementary pieces and the sort
std::vector<ContigWork> ingest_round(Run& run, RunStats& stats, const BamFile& bam, const std::string* names, size_t take) {
    const Cli& cli = run.cli;
    const Options& o = cli.o;
    std::vector<ContigWork> got(take);
    std::vector<std::unique_ptr<ContigIngest>> ing(take);
    std::vector<RealignQueue> queues(take);
    const bool on_device = !cli.ingest_only && !cli.no_realign;
    const PileupRoute route = effective_route(o.pileup, cli.no_realign);
    std::unique_ptr<RecordPileup> device_cells;                    // --pileup device: the round's CIGAR walks in one device call
    // --pileup resident: the round's walks (and realignment) in one device call whose cells stay there; the contigs it took are planned from headers, the
    // others (host_contigs) go the host route below
    std::unique_ptr<ResidentPileup> resident;
    std::vector<HeaderContig> planned(take);
    if (walk_on_device(route)) {
        const double tw = now_s();
        if (route == PileupRoute::Resident) resident.reset(new ResidentPileup(run.walker(), bam, run.vp, o, names, take, cli.no_realign ? nullptr : &run.fasta));
        else device_cells.reset(new RecordPileup(run.walker(), bam, run.vp, o, names, take, route == PileupRoute::Fused ? &run.fasta : nullptr));
        stats.add_walk(resident ? static_cast<const RoundWalk&>(*resident) : *device_cells, now_s() - tw, o.pileup);
    }
    const auto is_resident = [&](size_t i) { return resident && resident->on_table(i); };
    // a device segment (--inflate device): the records of a contig that keeps the host walk come down, one download per contig, and are decoded as a host segment's
    std::vector<std::unique_ptr<BamFile>> host_copy(take);
    if (bam.dev)
        for (size_t i = 0; i < take; ++i)
            if (!is_resident(i)) {
                const uint64_t before = bam.dev->bytes_down;
                host_copy[i].reset(new BamFile(host_copy_of_target(bam, names[i], run.n_threads)));
                stats.inflate_host_walk_bytes += bam.dev->bytes_down - before;
            }
    const auto records_of = [&](size_t i) -> const BamFile& { return host_copy[i] ? *host_copy[i] : bam; };
    parallel_for(take, run.n_threads, [&](size_t i) {
        const std::string& contig = names[i];
        if (is_resident(i)) { planned[i] = resident->plan(i); return; }
        const auto fa = run.fasta.find(contig);
        ing[i].reset(new ContigIngest(records_of(i), run.vp, o, contig, (fa != run.fasta.end() && !cli.no_realign) ? &fa->second : nullptr, on_device ? &queues[i] : nullptr, device_cells.get()));
    });
    device_cells.reset();
    std::vector<std::string> plan_texts(run.dump_pl.is_open() ? take : 0);
    if (run.dump_pl.is_open())
        parallel_for(take, run.n_threads, [&](size_t i) { plan_texts[i] = plan_text(names[i], is_resident(i) ? planned[i].plan : ing[i]->plan(), records_of(i)); });
    for (const std::string& t : plan_texts) run.dump_pl << t;
    if (resident) {
        // combine_frags on the device: one assemble call for the round (and one filter call under --ignore-monomorphic), before the next round's walk
        // rewrites the pileup buffers
        std::vector<HeaderContig*> hp(take, nullptr);
        for (size_t i = 0; i < take; ++i) if (is_resident(i)) hp[i] = &planned[i];
        // the handles keep positions (Frag::snp_pos_to_seq_pos) only where something reads them
        const bool keep_seq_pos = o.output_reads || !cli.dump_seq_pos.empty();
        resident->assemble(hp, run.reference_arith, keep_seq_pos, o.ignore_monomorphic, o.epsilon);
        stats.add_assembly(*resident);
        for (size_t i = 0; i < take; ++i) if (is_resident(i)) { ++stats.n_resident_contigs; stats.n_resident_merged += planned[i].merged_frags; }
    }
    if (on_device) {
        const double tr = now_s();
        RealignQueue all;
        for (RealignQueue& q : queues) all.append(std::move(q));
        stats.n_realign_device += all.size();
        realign_queue_on_device(run.walker(), all, o.realign_walk ? &o.walk : nullptr);
        stats.t_realign += now_s() - tr;
    }
    parallel_for(take, run.n_threads, [&](size_t i) {
        const std::string& contig = names[i];
        ContigWork& w = got[i];
        w.name = contig; w.out_dir = o.out_dir + "/" + contig;
        bool has_frags;                                                        // before the filter
        if (is_resident(i)) {
            // planned, assembled and filtered: the Frags are headers in the pileup's read order, the cells are behind the handle
            w.all_frags = std::move(planned[i].all_frags); w.frags_without_snps = std::move(planned[i].frags_without_snps);
            w.handle = std::move(planned[i].handle);
            w.resident_cells = planned[i].part_cells;
            has_frags = !planned[i].plan.frags.empty();
        } else {
            auto fr = ing[i]->finish();
            ing[i].reset();
            w.all_frags = std::move(fr.first); w.frags_without_snps = std::move(fr.second);
            has_frags = !w.all_frags.empty();
        }
        const auto sgp = run.vp.snp_to_genome_pos.find(contig);
        w.snp_to_genome_pos = sgp == run.vp.snp_to_genome_pos.end() ? nullptr : &sgp->second;
        // the contig directory is (re)made only for a contig that has fragments and SNPs, as floria.rs:263-281 does: with --overwrite a contig
        // that yields nothing in this run keeps what an earlier run wrote
        if (!cli.ingest_only && has_frags && w.snp_to_genome_pos) prepare_contig_dir(w.out_dir, o);
        const auto fa = run.fasta.find(contig);
        w.contig_len = fa == run.fasta.end() ? 0 : fa->second.size();
        if (is_resident(i)) return;
        std::sort(w.all_frags.begin(), w.all_frags.end());                     // floria.rs:289-293 (finish() yields them in this order already)
        for (size_t k = 0; k < w.all_frags.size(); ++k) w.all_frags[k].counter_id = k;
        if (o.ignore_monomorphic) w.all_frags = remove_monomorphic_allele(std::move(w.all_frags), o.epsilon);     // floria.rs:315-317
    });
    return got;
}

// --dump-frags: per contig "#CONTIG name n_frags n_snpless", a line per fragment (and its "#ORDER" where its set is not one walk's), "#SNPLESS" lines
std::string dump_frags_text(const std::vector<ContigWork>& work) {
    std::ostringstream dump;
    for (const ContigWork& w : work) {
        dump << "#CONTIG\t" << w.name << "\t" << w.all_frags.size() << "\t" << w.frags_without_snps.size() << "\n";
        for (const Frag& f : w.all_frags) {
            dump << f.id << "\t" << f.first_position << "\t" << f.last_position << "\t" << f.first_pos_base << "\t" << f.last_pos_base << "\t" << (f.is_paired ? 1 : 0);
            for (const auto& kv : f.seq_dict) dump << "\t" << kv.first << ":" << (int)kv.second << ":" << (int)f.qual_dict.at(kv.first);
            dump << "\n";
            if (f.other_set_order()) {          // the iteration order of its position set, replayed (tests compare it with the oracle's emulation)
                dump << "#ORDER";
                for (SnpPosition sp : f.positions_order()) dump << "\t" << sp;
                dump << "\n";
            }
        }
        for (const Frag& f : w.frags_without_snps) dump << "#SNPLESS\t" << f.id << "\t" << f.first_pos_base << "\t" << f.last_pos_base << "\t" << (f.seq_len[0] + f.seq_len[1]) << "\n";
    }
    return dump.str();
}

// --dump-seq-pos: per contig "#CONTIG name n_frags", then per fragment its id and snp:mate:seq_pos for every entry of snp_pos_to_seq_pos, ascending
std::string dump_seq_pos_text(const std::vector<ContigWork>& work) {
    std::ostringstream dump_sp;
    for (const ContigWork& w : work) {
        dump_sp << "#CONTIG\t" << w.name << "\t" << w.all_frags.size() << "\n";
        if (w.handle) {                              // header Frags: the same lines from the handle's SNP and SEQ_POS words (mate << 31 | seq_pos)
            const size_t R = w.all_frags.size();
            std::vector<uint32_t> ro(R + 1);
            auto get = [&](int field, std::vector<uint32_t>& v) {
                if (floria_hip_contig_download(w.handle.get(), field, v.data(), 4 * v.size()) != 0) throw Error(FLORIA_E_INVALID, std::string("--dump-seq-pos: ") + floria_hip_last_error());
            };
            get(FLORIA_FIELD_READ_OFF, ro);
            std::vector<uint32_t> snp(ro[R]), sp(ro[R]);
            get(FLORIA_FIELD_SNP, snp); get(FLORIA_FIELD_SEQ_POS, sp);
            for (size_t k = 0; k < R; ++k) {
                dump_sp << w.all_frags[k].id;
                for (uint32_t c = ro[k]; c < ro[k + 1]; ++c) dump_sp << "\t" << snp[c] << ":" << (sp[c] >> 31) << ":" << (sp[c] & 0x7fffffffu);
                dump_sp << "\n";
            }
            continue;
        }
        for (const Frag& f : w.all_frags) {
            dump_sp << f.id;
            for (const auto& kv : f.snp_pos_to_seq_pos) dump_sp << "\t" << kv.first << ":" << (int)kv.second.first << ":" << kv.second.second;
            dump_sp << "\n";
        }
    }
    return dump_sp.str();
}

// The contigs go through the stages in batches (floria_host.hpp, "many contigs at once"): the host stages of a batch run on -t
// threads, one contig per task; the device stages once per batch.  A batch is closed at batch_contigs contigs or batch_cells
// SNP calls, whichever comes first (the pinned staging buffer holds 6 bytes per call).
// ---- ingest (floria.rs:264-293) of the next batch of todo[done ..), one contig per task; `done` moves on
std::vector<ContigWork> ingest_batch(Run& run, RunStats& stats, const BamFile& bam, const std::vector<std::string>& todo, size_t& done) {
    const Cli& cli = run.cli;
    const double t0 = now_s();
    std::vector<ContigWork> work;
    uint64_t cells = 0;
    while (done < todo.size() && work.size() < cli.batch_contigs && cells < cli.batch_cells) {
        const size_t take = std::min({todo.size() - done, cli.batch_contigs - work.size(), std::max<size_t>(run.n_threads * 2, 2)});
        std::vector<ContigWork> got = ingest_round(run, stats, bam, &todo[done], take);
        done += take;
        for (ContigWork& w : got) {
            fprintf(stderr, "Number of reads passing filtering: %zu (%s)\n", w.all_frags.size(), w.name.c_str());
            if (w.all_frags.empty() || !w.snp_to_genome_pos) continue;
            if (!cli.ingest_only && w.contig_len == 0) throw Error(FLORIA_E_INVALID, "contig " + w.name + " is not in the reference fasta");
            for (const Frag& f : w.all_frags) cells += f.seq_dict.size();
            cells += w.resident_cells;                                         // (header Frags: the parts' cells, an upper bound of the merged count)
            work.push_back(std::move(w));
        }
    }
    if (run.dump.is_open()) run.dump << dump_frags_text(work);
    if (run.dump_sp.is_open()) run.dump_sp << dump_seq_pos_text(work);
    stats.t_ingest += now_s() - t0;
    return work;
}

// the device stages of a set of contigs on one context: S1 + hap graph in one pipelined call, LP + path peeling on the host (one contig per
// task), S2, COV / ERR / HAPQ of the final haplosets.  `tm` receives the wall seconds of the four stages.
void device_stages(Run& run, RunStats& stats, Session& session, std::vector<ContigWork>& part, size_t threads, double* tm) {
    const Cli& cli = run.cli;
    const Options& o = cli.o;
    double t1 = now_s();
    Batch batch(session, part, run.reference_arith);
    batch.generate_hap_graphs(o);
    if (run.dump_hd.is_open()) { const std::string t = batch.dump_handles(); std::lock_guard<std::mutex> g(run.dump_hd_mu); run.dump_hd << t; }
    tm[0] += now_s() - t1; t1 = now_s();
    parallel_for(part.size(), threads, [&](size_t i) {
        ContigWork& w = part[i];
        // (the uniqueness diagnostics cost O(E (V + E)) on top of the solve — 60-70 % more on layered graphs of thousands of columns — and feed
        // one summary line: only under --debug / --lp-report)
        LpInfo li;
        w.flows = solve_lp_graph(w.hap_graph, cli.lp_tie, cli.lp_report ? &li : nullptr);
        if (cli.lp_report) { ++stats.lp_contigs; stats.lp_not_unique += li.movable_edges != 0; stats.lp_edges += w.flows.size(); stats.lp_movable += li.movable_edges; }
        if (o.paths_resident) {                                              // the peeling alone: the union runs on the device (Batch::process_reads_for_final_parts)
            w.path_nodes = peel_disjoint_paths(w.hap_graph, w.flows, o);
            if (o.paths_keep_lists) { auto paths = unite_paths(w.hap_graph, w.path_nodes); w.path_parts = std::move(paths.first); w.path_ranges = std::move(paths.second); }      // (--debug prints them)
        } else {
        auto paths = get_disjoint_paths_rewrite(w.hap_graph, w.flows, o);
        w.path_parts = std::move(paths.first); w.path_ranges = std::move(paths.second);
        }
        if (cli.debug) write_debug_graph(w);
    });
    tm[1] += now_s() - t1; t1 = now_s();
    batch.process_reads_for_final_parts(o);
    tm[2] += now_s() - t1; t1 = now_s();
    batch.stats_and_hapq(o);
    tm[3] += now_s() - t1;
    stats.n_haplosets_by_handle += batch.haplosets_by_handle;
    stats.n_paths_joined += batch.paths_joined;
    if (batch.bytes_back) stats.resident_bytes_back += batch.bytes_back;    // (resident contigs exist with one device only: no other thread is here then)
}

// ---- the contigs of the batch dealt to the devices (longest first, by SNP calls), one host thread per device; every contig comes back
// to its place, so what follows (writers, the contig table) sees the batch in contig order whatever the dealing was
void deal_to_devices(Run& run, RunStats& stats, std::vector<ContigWork>& work, double* tm) {
    const auto& sessions = run.sessions;
    std::vector<double> cost(work.size());
    for (size_t i = 0; i < work.size(); ++i) { double c = 0; for (const Frag& f : work[i].all_frags) c += (double)f.seq_dict.size(); cost[i] = c; }
    const std::vector<uint32_t> owner = lpt_assign(cost, (uint32_t)sessions.size());
    std::vector<std::vector<ContigWork>> part(sessions.size());
    std::vector<std::vector<size_t>> origin(sessions.size());
    for (size_t i = 0; i < work.size(); ++i) { part[owner[i]].push_back(std::move(work[i])); origin[owner[i]].push_back(i); }
    std::vector<std::array<double, 4>> tms(sessions.size(), std::array<double, 4>{0., 0., 0., 0.});
    const size_t per_dev = std::max<size_t>(1, run.n_threads / sessions.size());
    parallel_for(sessions.size(), sessions.size(), [&](size_t d) { if (!part[d].empty()) device_stages(run, stats, *sessions[d], part[d], per_dev, tms[d].data()); });
    for (size_t d = 0; d < sessions.size(); ++d) {
        for (size_t k = 0; k < part[d].size(); ++k) work[origin[d][k]] = std::move(part[d][k]);
        for (int q = 0; q < 4; ++q) tm[q] = std::max(tm[q], tms[d][q]);        // (the devices run side by side: the slowest one counts)
    }
}

// ---- writers, one contig per task; the contig table in contig order
void write_batch(const Run& run, RunStats& stats, std::vector<ContigWork>& work) {
    const Options& o = run.cli.o;
    const double t0 = now_s();
    std::vector<std::string> rows(work.size());
    parallel_for(work.size(), run.n_threads, [&](size_t i) {
        ContigWork& w = work[i];
        w.snpless = get_frags_in_snpless_gaps(w.final_ranges, *w.snp_to_genome_pos, w.frags_without_snps, o.block_length, w.all_frags);
        rows[i] = write_contig_files(w, o);
    });
    for (const std::string& r : rows) append_contig_ploidy_row(o, r);
    stats.t_write += now_s() - t0;
}

}  // namespace

int main(int argc, char** argv) {
    floria_hip_init_env();                      // GPU_MAX_HW_QUEUES=12 unless set: the job groups' streams and the copy streams must not share hardware queues (read when HIP initialises)
    std::thread freer;                   // frees the Frags of the previous batch while the next one is ingested; joined before the process leaves main
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } freer_guard{freer};
    try {
        Cli cli = parse_args(argc, argv);
        if (cli.done) return 0;
        if (!cli.stitch_graph.empty()) { stitch_graph_tool(cli); return 0; }
        validate(cli);
        const Options& o = cli.o;

        RunStats stats;
        fprintf(stderr, "Preprocessing VCF/Reference\n");
        double tp = now_s();
        // the BAM is streamed: the records of a run of complete contigs at a time (about --bam-window-mb of inflated records), never the whole file
        // with an index beside it (unless --no-index) only the contigs that will be phased are read, each from its indexed offset
        BamStream stream(o.bam_file, std::max<size_t>(1, o.num_threads), !cli.no_index);
        double t_bam = now_s() - tp;
        // --estimate device: the estimate's pass needs the context, so the sessions are opened in front of it (their "arith" is set behind it, as always)
        const bool estimate_on_device = cli.estimate_device && (!cli.have_e || !cli.have_l);
        std::vector<std::unique_ptr<Session>> sessions;
        double t_device = 0.;
        if (estimate_on_device) { tp = now_s(); sessions = open_sessions(cli); t_device = now_s() - tp; }
        const Arithmetic arith = epsilon_policy(cli, stream, t_bam, estimate_on_device ? sessions[0]->ctx() : nullptr, stats);
        if (!cli.ingest_only) write_run_files(o, argc, argv, arith.run_note);
        const std::vector<std::string> contigs = stream.target_names();                 // get_contigs_to_phase (file_reader.rs:738-746)
        tp = now_s();
        const VcfProfile vp = get_vcf_profile(o.vcf_file, contigs);
        const std::map<std::string, std::string> fasta = get_fasta_seqs(o.reference_fasta);
        const double t_vcf = now_s() - tp;
        tp = now_s();
        if (!estimate_on_device) sessions = open_sessions(cli);
        for (auto& s : sessions) if (floria_hip_set_option(s->ctx(), "arith", arith.reference_arith ? 1 : 0) != 0) throw Error(FLORIA_E_INVALID, floria_hip_last_error());
        fprintf(stderr, "Preprocessing: BAM header%s %.3fs, VCF + FASTA %.3fs, device %.3fs\n", (!cli.have_e || !cli.have_l) ? " + parameter estimate" : "", t_bam, t_vcf,
                t_device + now_s() - tp);

        Run run(cli, vp, fasta, contigs, sessions, arith.reference_arith);
        if (!cli.ingest_only) check_contigs_in_fasta(run);
        if (!stream.index_path().empty()) {           // the predicate of contigs_of_segment, which still sees every target and gives its warning
            std::vector<int32_t> tids;
            for (size_t tid = 0; tid < contigs.size(); ++tid) if (run.listed(contigs[tid]) && run.enough_snps(contigs[tid])) tids.push_back((int32_t)tid);
            stream.select(tids);
        }
        if (cli.inflate_device) stream.inflate_on_device(run.walker().ctx());       // from here on the host inflates nothing: segments are planned from member headers
        BamFile bam;                                  // the current segment: every record of the contigs [tid_begin, tid_end)
        for (;;) {
            { const double ts = now_s(); const bool more = stream.next(bam, cli.bam_window); stats.t_stream += now_s() - ts; if (!more) break; }
            ++stats.n_segments; stats.n_records += bam.records.size();
            const std::vector<std::string> todo = contigs_of_segment(run, stats, bam);
            size_t done = 0;
            while (done < todo.size()) {
                std::vector<ContigWork> work = ingest_batch(run, stats, bam, todo, done);
                if (cli.ingest_only || work.empty()) continue;
                ++stats.n_batches;
                if (run.reference_arith) stats.add_set_orders(work);
                double tm[4] = {0., 0., 0., 0.};
                if (sessions.size() == 1) device_stages(run, stats, *sessions[0], work, run.n_threads, tm);
                else deal_to_devices(run, stats, work, tm);
                stats.t_s1 += tm[0]; stats.t_stitch += tm[1]; stats.t_s2 += tm[2]; stats.t_stats += tm[3];
                write_batch(run, stats, work);
                // the Frags of a batch are millions of small objects: freeing them goes to a thread of its own, the next batch's ingest does not wait for it
                for (ContigWork& w : work) w.handle.reset();                           // (device memory goes back on this thread: a context takes one host thread at a time)
                if (freer.joinable()) freer.join();
                freer = std::thread([w = std::make_shared<std::vector<ContigWork>>(std::move(work))]() mutable { w.reset(); });
            }
        }       // (next segment of the BAM)
        stats.report(cli, stream, run.reference_arith);
        // everything is written and closed: leave without tearing down the records, maps and sequences one by one (seconds for a large BAM)
        run.close_dumps();
        sessions.clear();
        // every output stream of this run was scoped to the function that wrote it and is closed; stdio is flushed here.  What is left are the records,
        // maps and sequences of the inputs, whose node-by-node teardown takes seconds for a large run: the process leaves without it (the freer of the
        // last batch is abandoned with it, on the success path only).
        fflush(nullptr);
        if (freer.joinable()) freer.detach();
        std::_Exit(0);
    } catch (const Error& e) {
        fprintf(stderr, "floria-hip: error: %s\n", e.what());
        return 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "floria-hip: error: %s\n", e.what());
        return 1;
    }
    return 0;
}
