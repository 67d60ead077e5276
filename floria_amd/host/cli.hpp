// cli.hpp — floria-hip's command line: the options of the library's host side plus the driver's own settings, and the three test tools that need no GPU (cli.cpp)
#pragma once
#include <string>
#include <vector>

#include "floria_host.hpp"

namespace floria {

struct Cli {
    Options o;
    bool have_e = false, have_l = false;
    std::string dump_frags, dump_seq_pos, dump_plan, dump_handles, dump_estimate;
    bool estimate_device = false;                  // --estimate device: the -e / -l estimate reads device segments (floria_hip_blob_estimate)
    size_t batch_contigs = 4096;         // --batch-contigs
    uint64_t batch_cells = 256ull << 20; // --batch-cells (1.5 GB of pinned staging)
    bool ingest_only = false, no_realign = false, have_realign = false;
    std::string stitch_graph;
    bool stitch_paths = false;
    LpTie lp_tie = LpTie::First;         // --lp-tie first|last: which optimal vertex of the stitching LP is used where the optimum is not unique (stitch.cpp)
    bool lp_report = false;              // --lp-report (implied by --debug): count the edges whose flow differs in another optimal solution of the stitching LP
    bool debug = false;                  // --debug / --trace: per contig, debug_graph.txt (hap graph, LP flows, joined paths) next to the outputs
    std::vector<int> devices;            // --devices: the GPUs the contigs of a batch are dealt to (empty: --device alone)
    size_t bam_window = (size_t)512 << 20;   // --bam-window-mb: inflated BAM bytes held at a time (more only when one contig alone is larger)
    bool no_index = false;               // --no-index: stream the whole BAM in file order even when an index lies beside it
    bool inflate_device = false;         // --inflate device: the BGZF members of a segment are inflated, and their records read, on the device (--pileup resident only)
    std::string arith_opt = "auto";      // --arith auto|reference|canonical: the reference's running f64 sums (device mode arith = 1) or the exact (Q24, #eps) form; auto = reference
                                         // arithmetic exactly when epsilon is not a multiple of 2^-10 (where the two are different functions)
    bool eps_round = false;              // --epsilon-round: round an auto-estimated -e to a multiple of 2^-10 (default: used as estimated, like the reference)
    bool done = false;                   // -h, --vcf-profile or --lpt-assign has answered the command line: nothing is left to run
};

// Throws Error for an unknown option, a missing or malformed value and the options floria has and this build has not.  --vcf-profile and --lpt-assign act where
// they stand in argv and take the rest of it; --stitch-graph is only noted: it runs once the whole line is parsed, so a later --lp-tie still counts.
Cli parse_args(int argc, char** argv);
// the refusals that need more than one option, before anything is read
void validate(const Cli& cli);
// (tests) --stitch-graph FILE: N / E lines of a hap graph -> U / F / P lines on stdout; with --stitch-paths also Q lines: every path's nodes
void stitch_graph_tool(const Cli& cli);

}  // namespace floria
