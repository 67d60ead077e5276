// cli.cpp — floria-hip's command line (cli.hpp): usage, the option loop, the cross-option refusals and the test tools that need no GPU
#include "cli.hpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

namespace floria {

namespace {

void usage() {
    fputs("floria-hip - strain phasing for short or long-read shotgun metagenomic sequencing (MI355X build of floria's phasing path).\n\n"
          "Example usage :\nfloria-hip -b bamfile.bam -v vcffile.vcf -r reference.fa -o results -t 10\n\n"
          "floria's options, same meaning:\n"
          "  -b FILE  sorted BAM            -v FILE  VCF (plain / gz / bgz) or BCF with the SNPs     -r FILE  reference fasta\n"
          "  -o DIR   output directory [floria_out_dir]       --overwrite   reuse an existing one    -t N  host threads [10]\n"
          "  -e X     allele error rate epsilon [estimated]   -l N  block length in bases [estimated]   -d X  SNP density filter [0.0005]\n"
          "  -n N     beam solutions [10]    -p N  maximum ploidy [5; this build: 1..16]    -s 1|2|3  ploidy sensitivity [2]    --no-stop-heuristic\n"
          "  -m N     MAPQ cutoff [15]       -G / --contigs NAME..  only these contigs      --snp-count-filter N [100]\n"
          "  -X / --no-supp  ignore supplementary alignments      --supp-aln-dist-cutoff N [40000]      --ignore-monomorphic\n"
          "  --output-reads [--gzip-reads] [--extra-trimming]     --debug / --trace\n"
          "this build's own:\n"
          "  --device N | --devices 0-7 | 0,2,5   GPU(s); contigs of a batch are dealt to them, files do not depend on it\n"
          "  --batch-contigs N [4096]  --batch-cells N [2^28]   contigs taken through the device stages together\n"
          "  --bam-window-mb N [512]   inflated BAM records held in memory at a time\n"
          "  an index beside the BAM (X.bam.bai, then X.bai) is used when present: only the contigs to be phased (-G, --snp-count-filter) are read, each from its indexed offset\n"
          "  --no-index        ignore the index: stream the whole file in order, as when there is none\n"
          "  --arith auto|reference|canonical   how sums of epsilon terms are rounded when -e is not a multiple of 2^-10: 'reference' = floria's running f64 sums\n"
          "                 in its hash containers' iteration order (as far as that order can be emulated), 'canonical' = every sum rounded once; auto [default] =\n"
          "                 reference, except for batches with fragments merged from mates / supplementary alignments or under --ignore-monomorphic\n"
          "  --epsilon-round   round an ESTIMATED -e to a multiple of 2^-10 (there both arithmetics are the same function)\n"
          "  --lp-tie first|last, --lp-report   which optimal vertex of the stitching LP is used where the optimum is not unique, and how often that is\n"
          "  --no-realign      skip the re-alignment of the reads' bases around SNPs\n"
          "  --pileup host|device|fused|resident   where alignment records become SNP calls (the CIGAR walk): on the host threads [default] or in one device call per ingest\n"
          "                    round; fused: that device call also re-aligns the calls (instead of the host loop that queues windows for the device); resident: the calls\n"
          "                    never come back - fragments are planned from the records' headers and assembled, filtered (--ignore-monomorphic) and phased on the device,\n"
          "                    the writers ask it for allele tables and read trims (one device only; no --dump-frags).  Same files\n"
          "  --inflate host|device   where the BGZF members of the BAM are inflated: host [default] = on the host threads, the inflated records uploaded for the walk; device =\n"
          "                    the compressed members of a segment go up as they lie in the file, are inflated there (floria_hip_inflate_bgzf) and the records are read where\n"
          "                    they are walked: the host sees a header-sized table of them (floria_hip_blob_records_opt), --output-reads' bases come back in one call per\n"
          "                    ingest round (floria_hip_blob_sequences).  Needs --pileup resident (no other route leaves the record bytes unread on the host); the BAM header\n"
          "                    and the -e / -l estimate are still inflated on the host (the estimate unless --estimate device).  Same files\n"
          "  --estimate host|device   where the -e / -l estimate (made when -e or -l is not given) reads the records: host [default] = the file's first segments are inflated\n"
          "                    and decoded on the host threads; device = they are inflated on the device as under --inflate device and the sampled pileup columns are\n"
          "                    counted there (floria_hip_blob_estimate): header-sized data comes back.  Needs --inflate device (the pass reads the blobs of that route);\n"
          "                    accepted and unused when both -e and -l are given.  Same estimate, same files\n"
          "  --haplosets host|resident   where the haplosets live between S2 and the writers: host [default] = S2 returns the group lists and the four calls behind it\n"
          "                    (COV / ERR, HAPQ, allele tables, read trims) take them up again; resident = S2 splits and sorts on the device and keeps the haplosets there\n"
          "                    (floria_hip_reassign_batch_resident), the lists come back once for the writers and the four calls take the handle.  Any --pileup route.  Same files\n"
          "  --paths host|resident   where the reads of a hap-graph path are united: host [default] = S1 returns every block's read list, the nodes hold their reads and the\n"
          "                    path peeling unites them; resident = the peeling returns node lists, floria_hip_join_paths unites the reads on the S1 batch that is still on the\n"
          "                    device and S2 takes that handle (floria_hip_reassign_haplosets_resident): no read list comes down (unless --debug) or goes up.  Implies\n"
          "                    --haplosets resident.  Any --pileup route.  Same files\n"
          "  --realign exact | block:STEP,RULE,TIE   how that re-alignment scores a window: exact [default] = the exact affine-gap alignment; block:... = a walk of a fixed\n"
          "                 8 x 8 block over the alignment matrix, shifted by STEP = 1 | 2 | 4 | 8 cells towards the larger border by RULE = max | sum, ties going\n"
          "                 TIE = right | down (e.g. block:8,max,right).  floria's block-aligner is a heuristic of this kind; which member is unknown, so one must be named\n"
          "where this build is not floria (DESIGN.md sections 6 and 7):\n"
          "  * re-alignment around SNPs is the EXACT affine-gap alignment of the 32-base windows; floria's block-aligner is a banded heuristic of it (calls can differ;\n"
          "    --realign block:... selects one of 16 fixed-block walks instead, none of which is known to be block-aligner's)\n"
          "  * the stitching LP is solved exactly as a min-cost flow: the same optimal value as floria's simplex, possibly another optimal vertex (short reads: haplosets can differ)\n"
          "  * hash-set iteration orders decide ties in floria (visiting order of the final reassignment, the read dropped at a haplogroup split): here ascending read order\n"
          "  * not supported: -H / --hybrid, --reassign-short, --bin-by-cov (hidden or beta in floria)\n", stderr);
}

// (tests) --vcf-profile FILE contig ... -> "contig n_snps" and one "pos alleles" line per SNP, no GPU needed
void vcf_profile_tool(const std::string& vcf, const std::vector<std::string>& names) {
    const VcfProfile vp = get_vcf_profile(vcf, names);
    for (const auto& kv : vp.snp_to_genome_pos) {
        printf("#%s\t%zu\n", kv.first.c_str(), kv.second.size());
        const auto& pam = vp.vcf_pos_allele_map.at(kv.first);
        for (GnPosition g : kv.second) { printf("%zu\t", (size_t)g); for (Genotype x : pam.at(g)) putchar((char)x); putchar('\n'); }
    }
}

// (tests) --lpt-assign world cost cost ... -> the device of every item, no GPU needed
void lpt_assign_tool(uint32_t world, const std::vector<double>& costs) {
    for (uint32_t d : lpt_assign(costs, world)) printf("%u\n", d);
}

}  // namespace

Cli parse_args(int argc, char** argv) {
    Cli cli;
    Options& o = cli.o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) throw Error(FLORIA_E_INVALID, "missing value for " + a); return argv[++i]; };
        if (a == "-b") o.bam_file = val();
        else if (a == "-v") o.vcf_file = val();
        else if (a == "-r") o.reference_fasta = val();
        else if (a == "-o" || a == "--output-dir") o.out_dir = val();
        else if (a == "-t" || a == "--threads") o.num_threads = (size_t)std::stoul(val());
        else if (a == "-e" || a == "--epsilon") { o.epsilon = std::stod(val()); cli.have_e = true; }
        else if (a == "-n" || a == "--beam-solns") o.max_number_solns = (size_t)std::stoul(val());
        else if (a == "-p" || a == "--max-ploidy") {
            o.max_ploidy = (size_t)std::stoul(val());
            if (o.max_ploidy < 1 || o.max_ploidy > FLORIA_MAX_PLOIDY)           // (the reference takes any -p; its default is 5.  include/floria_hip.h: the optimise kernel packs partitions into 4 bits)
                throw Error(FLORIA_E_UNSUPPORTED, "-p " + std::to_string(o.max_ploidy) + ": this build phases ploidies 1 to " + std::to_string(FLORIA_MAX_PLOIDY));
        }
        else if (a == "-l" || a == "--block-length") { o.block_length = (size_t)std::stoul(val()); cli.have_l = true; }
        else if (a == "-d" || a == "--snp-density") o.snp_density = std::stod(val());
        else if (a == "-s" || a == "--ploidy-sensitivity") o.ploidy_sensitivity = (uint8_t)std::stoul(val());
        else if (a == "-m" || a == "--mapq-cutoff") o.mapq_cutoff = (uint8_t)std::stoul(val());
        else if (a == "--snp-count-filter") o.snp_count_filter = (size_t)std::stoul(val());
        else if (a == "--supp-aln-dist-cutoff") o.supp_aln_dist_cutoff = std::stoll(val());
        else if (a == "-X" || a == "--no-supp") o.dont_use_supp_aln = true;
        else if (a == "--no-stop-heuristic") o.stopping_heuristic = false;
        else if (a == "--overwrite") o.overwrite = true;
        else if (a == "--debug" || a == "--trace") { cli.debug = true; cli.lp_report = true; }
        else if (a == "--lp-report") cli.lp_report = true;
        else if (a == "--lp-tie") { const std::string v = val(); if (v != "first" && v != "last") throw Error(FLORIA_E_INVALID, "--lp-tie takes first or last"); cli.lp_tie = v == "last" ? LpTie::Last : LpTie::First; }
        else if (a == "-q") {}
        else if (a == "-G" || a == "--contigs") { while (i + 1 < argc && argv[i + 1][0] != '-') o.list_to_phase.push_back(argv[++i]); }
        else if (a == "--device") o.device = std::stoi(val());
        else if (a == "--epsilon-as-estimated") {}                          // (the default since round 4; accepted for older command lines)
        else if (a == "--epsilon-round") cli.eps_round = true;
        else if (a == "--arith") { cli.arith_opt = val(); if (cli.arith_opt != "auto" && cli.arith_opt != "reference" && cli.arith_opt != "canonical") throw Error(FLORIA_E_INVALID, "--arith takes auto, reference or canonical"); }
        else if (a == "--bam-window-mb") cli.bam_window = std::max<size_t>(1, std::stoul(val())) << 20;
        else if (a == "--bam-window-kb") cli.bam_window = std::max<size_t>(1, std::stoul(val())) << 10;       // (tests: many segments on a small file)
        else if (a == "--no-index") cli.no_index = true;
        else if (a == "--devices") {                                 // "0-7", "0,2,5", "0-3,6"; a device may be named twice (two contexts on it)
            std::stringstream ls(val());
            std::string item;
            while (std::getline(ls, item, ',')) {
                const size_t dash = item.find('-', 1);
                const int lo = std::stoi(item.substr(0, dash)), hi = dash == std::string::npos ? lo : std::stoi(item.substr(dash + 1));
                if (lo < 0 || hi < lo || hi - lo > 1024) throw Error(FLORIA_E_INVALID, "--devices: bad range " + item);
                for (int d = lo; d <= hi; ++d) cli.devices.push_back(d);
            }
            if (cli.devices.empty()) throw Error(FLORIA_E_INVALID, "--devices: empty list");
        }
        else if (a == "--vcf-profile") {
            const std::string vcf = val();
            std::vector<std::string> names;
            while (i + 1 < argc) names.push_back(argv[++i]);
            vcf_profile_tool(vcf, names);
            cli.done = true;
            return cli;
        }
        else if (a == "--lpt-assign") {
            const uint32_t world = (uint32_t)std::stoul(val());
            std::vector<double> costs;
            while (i + 1 < argc) costs.push_back(std::stod(argv[++i]));
            lpt_assign_tool(world, costs);
            cli.done = true;
            return cli;
        }
        else if (a == "--batch-contigs") cli.batch_contigs = std::max<size_t>(1, std::stoul(val()));       // contigs per device batch
        else if (a == "--batch-cells") cli.batch_cells = std::max<uint64_t>(1, std::stoull(val()));        // SNP calls per device batch
        else if (a == "--dump-frags") cli.dump_frags = val();
        else if (a == "--dump-seq-pos") cli.dump_seq_pos = val();      // (tests) Frag::snp_pos_to_seq_pos of every fragment, in --dump-frags' order
        else if (a == "--no-realign") cli.no_realign = true;                   // (tests) keep the alleles as called
        else if (a == "--realign") { parse_realign_spec(val(), o); cli.have_realign = true; }
        else if (a == "--pileup") {
            const std::string v = val();
            if (v != "host" && v != "device" && v != "fused" && v != "resident")
                throw Error(FLORIA_E_INVALID, "--pileup takes host or device (or fused: device, and the calls re-aligned there; or resident: the calls stay on the device), not '" + v + "'");
            o.pileup = v == "device" ? PileupRoute::Device : v == "fused" ? PileupRoute::Fused : v == "resident" ? PileupRoute::Resident : PileupRoute::Host;
        }
        else if (a == "--inflate") {
            const std::string v = val();
            if (v != "host" && v != "device") throw Error(FLORIA_E_INVALID, "--inflate takes host or device, not '" + v + "'");
            cli.inflate_device = v == "device";
        }
        else if (a == "--estimate") {
            const std::string v = val();
            if (v != "host" && v != "device") throw Error(FLORIA_E_INVALID, "--estimate takes host or device, not '" + v + "'");
            cli.estimate_device = v == "device";
        }
        else if (a == "--haplosets") {
            const std::string v = val();
            if (v != "host" && v != "resident") throw Error(FLORIA_E_INVALID, "--haplosets takes host or resident, not '" + v + "'");
            o.haplosets_resident = v == "resident";
        }
        else if (a == "--paths") {
            const std::string v = val();
            if (v != "host" && v != "resident") throw Error(FLORIA_E_INVALID, "--paths takes host or resident, not '" + v + "'");
            o.paths_resident = v == "resident";
        }
        else if (a == "--stitch-paths") cli.stitch_paths = true;      // (tests, with --stitch-graph) also one Q line per path: its nodes
        else if (a == "--dump-plan") cli.dump_plan = val();            // (tests, with --ingest-only) the fragment plan of every contig: needs no GPU under --pileup host
        else if (a == "--dump-estimate") cli.dump_estimate = val();    // (tests, with --ingest-only) the sampled columns and the state of the -e / -l estimate: needs no GPU under --estimate host
        else if (a == "--dump-handles") cli.dump_handles = val();      // (tests) the resident arrays of every contig of every batch, whichever route made the handle
        else if (a == "--ingest-only") cli.ingest_only = true;          // (tests) stop after ingest: needs no GPU
        else if (a == "--stitch-graph") cli.stitch_graph = val();       // (tests) N / E lines of a hap graph -> F / P lines on stdout: needs no GPU
        else if (a == "-h" || a == "--help") { usage(); cli.done = true; return cli; }
        else if (a == "--output-reads") o.output_reads = true;
        else if (a == "--gzip-reads") o.gzip = true;
        else if (a == "--extra-trimming") o.trim_reads = true;
        else if (a == "--ignore-monomorphic") o.ignore_monomorphic = true;
        else if (a == "-H" || a == "--hybrid" || a == "--reassign-short" || a == "--bin-by-cov")
            throw Error(FLORIA_E_UNSUPPORTED, "option " + a + " of floria is not supported by floria-hip");
        else throw Error(FLORIA_E_INVALID, "unknown option " + a);
    }
    if (o.paths_resident) { o.haplosets_resident = true; o.paths_keep_lists = cli.debug; }
    return cli;
}

void validate(const Cli& cli) {
    const Options& o = cli.o;
    if (cli.no_realign && cli.have_realign && o.realign_walk) throw Error(FLORIA_E_INVALID, "--no-realign and --realign " + realign_spec(o) + " exclude each other");
    if (o.pileup == PileupRoute::Resident && cli.devices.size() > 1)
        throw Error(FLORIA_E_UNSUPPORTED, "--pileup resident runs on one device: the handles live on the context that walked the records, and dealing the contigs of a batch to "
                                          "devices (--devices) would have to precede the walk");
    if (o.pileup == PileupRoute::Resident && !cli.dump_frags.empty())
        throw Error(FLORIA_E_UNSUPPORTED, "--dump-frags is not available under --pileup resident: the quality bytes are folded into weights on the device and cannot be printed "
                                          "(--dump-handles and --dump-seq-pos work)");
    if (cli.inflate_device && o.pileup != PileupRoute::Resident)
        throw Error(FLORIA_E_UNSUPPORTED, "--inflate device needs --pileup resident: only that route leaves the record bytes unread on the host (every other route walks or "
                                          "merges the records' CIGARs, bases and qualities there, so they would have to come back down)");
    if (cli.estimate_device && !cli.inflate_device)
        throw Error(FLORIA_E_UNSUPPORTED, "--estimate device needs --inflate device: the estimate then reads the blobs that route inflates on the device (under --inflate host "
                                          "the records are inflated on the host anyway, and its estimate reads them there)");
    if (!cli.dump_plan.empty() && !cli.ingest_only) throw Error(FLORIA_E_INVALID, "--dump-plan needs --ingest-only");
    if (!cli.dump_estimate.empty() && !cli.ingest_only) throw Error(FLORIA_E_INVALID, "--dump-estimate needs --ingest-only");
    if (!cli.dump_estimate.empty() && cli.have_e && cli.have_l) throw Error(FLORIA_E_INVALID, "--dump-estimate needs the estimate: leave out -e or -l");
    if (o.bam_file.empty()) throw Error(FLORIA_E_INVALID, "Must input a BAM file.");
    if (o.vcf_file.empty() || o.reference_fasta.empty()) throw Error(FLORIA_E_INVALID, "-v and -r are required");
    if (!(o.ploidy_sensitivity >= 1 && o.ploidy_sensitivity <= 3)) throw Error(FLORIA_E_INVALID, "Ploidy sensitivty option must be between 1 and 3");
}

void stitch_graph_tool(const Cli& cli) {
    // hap graph in the format of debug_graph.txt (N: column row id cov lo hi reads..., E: column row row2 weight)
    std::ifstream in(cli.stitch_graph);
    if (!in) throw Error(FLORIA_E_INVALID, "cannot open " + cli.stitch_graph);
    std::vector<std::vector<HapNode>> hg;
    std::vector<Frag> frags;
    std::vector<std::vector<std::vector<size_t>>> node_reads;
    std::string tag;
    size_t max_read = 0;
    struct EdgeIn { size_t c, r, r2; double w; };
    std::vector<EdgeIn> edges;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> tag;
        if (tag == "N") {
            size_t c, r, id; double cov; SnpPosition lo, hi;
            ls >> c >> r >> id >> cov >> lo >> hi;
            if (hg.size() <= c) { hg.resize(c + 1); node_reads.resize(c + 1); }
            if (hg[c].size() <= r) { hg[c].resize(r + 1); node_reads[c].resize(r + 1); }
            HapNode& n = hg[c][r];
            n.column = c; n.row = r; n.id = id; n.cov = cov; n.snp_endpoints = {lo, hi};
            size_t x;
            while (ls >> x) { node_reads[c][r].push_back(x); max_read = std::max(max_read, x + 1); }
        } else if (tag == "E") { EdgeIn e; ls >> e.c >> e.r >> e.r2 >> e.w; edges.push_back(e); }
    }
    frags.resize(max_read);
    for (size_t i = 0; i < max_read; ++i) frags[i].counter_id = i;
    for (size_t c = 0; c < hg.size(); ++c) for (size_t r = 0; r < hg[c].size(); ++r) for (size_t x : node_reads[c][r]) hg[c][r].frag_set.push_back(&frags[x]);
    for (const EdgeIn& e : edges) { hg[e.c][e.r].out_edges.push_back({e.r2, e.w}); hg[e.c + 1][e.r2].in_edges.push_back({e.r, e.w}); }
    LpInfo li;
    const FlowUpVec fl = solve_lp_graph(hg, cli.lp_tie, &li);
    const std::vector<PeeledPath> peeled = peel_disjoint_paths(hg, fl, cli.o);
    auto paths = unite_paths(hg, peeled);
    printf("U\t%lld\t%zu\n", (long long)li.cost, li.movable_edges);
    for (const FlowUpdate& f : fl) printf("F\t%zu\t%zu\t%zu\t%.17g\n", f.n1.first, f.n1.second, f.n2.second, f.flow);
    for (size_t k = 0; k < paths.first.size(); ++k) {
        printf("P\t%u\t%u", paths.second[k].first, paths.second[k].second);
        for (const Frag* f : paths.first[k]) printf("\t%zu", f->counter_id);
        printf("\n");
    }
    if (cli.stitch_paths)                                              // path k's range and its nodes (column:row), sink first
    for (const PeeledPath& p : peeled) {
        printf("Q\t%u\t%u", p.ends.first, p.ends.second);
        for (const auto& cr : p.nodes) printf("\t%zu:%zu", cr.first, cr.second);
        printf("\n");
    }
}

}  // namespace floria
