// floria_host.hpp — C++ host mirror of the two reference call sites, on top of the C ABI (include/floria_hip.h).
//
// The reference is compiled code (Rust) and there is no Rust toolchain in this image, so the host side above the C ABI is
// C++ with the reference's names, argument meaning and error behaviour:
//   floria::get_range_with_lengths          utils_frags.rs:405-463
//   floria::generate_hap_graph              graph_processing.rs:325-372   (get_local_hap_blocks per block -> process_chunks ->
//                                                                          update_hap_graph, all on the device)
//   floria::process_reads_for_final_parts   part_block_manip.rs:174-274
//   floria::solve_lp_graph                  solve_flow.rs:195-290          (host; exact min-cost flow, see stitch.cpp)
//   floria::get_disjoint_paths_rewrite      graph_processing.rs:462-750    (host)
//   floria::get_frags_in_snpless_gaps       part_block_manip.rs:622-675    (host)
//   floria::write_outputs                   file_writer.rs:21-84,151-165,308-369,699-993   (.vartigs, .haplosets, vartig_info.txt,
//                                                                          reads_without_snps.tsv, contig_ploidy_info.tsv)
//   floria::get_vcf_profile, get_contigs_to_phase, get_frags_from_bamvcf_rewrite, get_fasta_seqs   file_reader.rs (ingest.cpp)
// Where the reference panics or exits (malformed VCF positions, :422-425) these functions throw floria::Error carrying the
// library's message.  There is no CPU fallback: constructing a Session without a usable MI355X throws.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <iosfwd>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "../../include/floria_hip.h"

namespace floria {

typedef size_t GnPosition;          // types_structs.rs:11
typedef uint32_t SnpPosition;       // types_structs.rs:12
typedef uint8_t Genotype;           // types_structs.rs:13

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// --pileup host | device | fused | resident: where the CIGAR walk that turns alignment records into SNP calls runs
//   Host      frag_from_record on the host threads (default)
//   Device    floria_hip_pileup_records, one call per ingest round (RecordPileup)
//   Fused     Device, and the calls are realigned by the same device call (floria_hip_pileup_records_realign) instead of by realign()
//   Resident  the walk (and the realignment) by floria_hip_pileup_records_resident, the fragments assembled on the device from a plan made of headers
//             (floria_hip_assemble_contigs_opt): the host holds header-only Frags and a handle per contig, no cell comes back (ResidentPileup)
enum class PileupRoute { Host, Device, Fused, Resident };
inline const char* route_name(PileupRoute r) { return r == PileupRoute::Host ? "host" : r == PileupRoute::Device ? "device" : r == PileupRoute::Fused ? "fused" : "resident"; }
// the round's CIGAR walks are one device call
inline bool walk_on_device(PileupRoute r) { return r != PileupRoute::Host; }
// --ingest-only needs no device, unless the walk runs there
inline bool needs_session(PileupRoute r, bool ingest_only) { return !ingest_only || walk_on_device(r); }
// the calls are realigned by the device call that walked them (the host loop that queues windows then sees only the contigs that kept the host walk)
inline bool realigned_behind_walk(PileupRoute r, bool no_realign) { return !no_realign && (r == PileupRoute::Fused || r == PileupRoute::Resident); }
// --pileup fused --no-realign is --pileup device
inline PileupRoute effective_route(PileupRoute r, bool no_realign) { return r == PileupRoute::Fused && no_realign ? PileupRoute::Device : r; }

// The hot-path fields of `Options` (types_structs.rs:20-51) with the CLI defaults (parse_cmd_line.rs)
struct Options {
    std::string bam_file, vcf_file, reference_fasta, out_dir = "floria_out_dir";     // -b -v -r -o
    double epsilon = 0.04;              // -e (auto-estimated from the BAM when absent, parse_cmd_line.rs:72-90)
    size_t max_number_solns = 10;       // -n
    size_t max_ploidy = 5;              // -p
    size_t block_length = 15000;        // -l (auto-estimated when absent)
    double snp_density = 0.0005;        // -d
    bool stopping_heuristic = true;     // !--no-stop-heuristic
    uint8_t ploidy_sensitivity = 2;     // -s
    size_t num_threads = 10;            // -t (accepted; the blocks run on the GPU)
    size_t snp_count_filter = 100;      // --snp-count-filter
    uint8_t mapq_cutoff = 15;           // -m
    int64_t supp_aln_dist_cutoff = 40000;   // --supp-aln-dist-cutoff
    bool dont_use_supp_aln = false;     // -X
    bool overwrite = false;             // --overwrite
    std::vector<std::string> list_to_phase;   // -G
    bool reassign_short = false;        // hidden flag; not supported (part_block_manip.rs:235-270)
    bool output_reads = false;          // --output-reads: fastq of every haploset's reads (file_writer.rs:370-560)
    bool gzip = false;                  // --gzip-reads
    bool trim_reads = false;            // --extra-trimming
    bool ignore_monomorphic = false;    // --ignore-monomorphic (utils_frags.rs:713-772)
    int device = 0;
    // --realign exact | block:STEP,RULE,TIE: how alignment::realign scores a window.  false: the exact affine-gap DP (default); true: the member `walk` of the
    // fixed-block walk family (floria_hip_realign_walk on the device, walk_affine_score on the host)
    bool realign_walk = false;
    floria_realign_walk walk = {8, 8, 0, 0};
    PileupRoute pileup = PileupRoute::Host;   // --pileup
    bool haplosets_resident = false;    // --haplosets resident: S2 by floria_hip_reassign_batch_resident, one download, and the handle to the four consumers (Batch)
    // --paths resident: the path peeling returns node lists, the reads of a path are united on the device (floria_hip_join_paths) and S2 takes that handle
    // (floria_hip_reassign_haplosets_resident); S1 then returns no read list ("s1_no_lists") unless paths_keep_lists (--debug prints the nodes' reads)
    bool paths_resident = false, paths_keep_lists = false;
};
// "exact" | "block:STEP,RULE,TIE" (STEP 1 | 2 | 4 | 8, RULE max | sum, TIE right | down) -> options.realign_walk / options.walk; anything else throws with the grammar
void parse_realign_spec(const std::string& spec, Options& options);
std::string realign_spec(const Options& options);                                     // the spelling parse_realign_spec accepts
// score of one member of the fixed-block walk family (block 8; scripts/probes/block_walk.c: walk_score), the host twin of floria_hip_realign_walk
int walk_affine_score(const unsigned char* q, int nq, const unsigned char* r, int nr, const floria_realign_walk& walk);

// The per-read maps of the reference's Frag (FxHashMap<SnpPosition, _>, types_structs.rs:72-84) as a sorted vector with std::map's
// interface: a read has ~100 entries, inserted in ascending order by the CIGAR walk — one allocation instead of one tree node per entry
// (std::map made the ingest of 200 k long reads spend its time in malloc/free: 53 M nodes), iteration ascends like the BTreeMap-like uses need.
template <class K, class V> class FlatMap {
public:
    typedef std::pair<K, V> value_type;
    typedef typename std::vector<value_type>::iterator iterator;
    typedef typename std::vector<value_type>::const_iterator const_iterator;
    typedef typename std::vector<value_type>::const_reverse_iterator const_reverse_iterator;
    iterator begin() { return v_.begin(); }
    iterator end() { return v_.end(); }
    const_iterator begin() const { return v_.begin(); }
    const_iterator end() const { return v_.end(); }
    const_reverse_iterator rbegin() const { return v_.rbegin(); }
    const_reverse_iterator rend() const { return v_.rend(); }
    size_t size() const { return v_.size(); }
    bool empty() const { return v_.empty(); }
    void clear() { v_.clear(); }
    iterator lower_bound(const K& k) { return std::lower_bound(v_.begin(), v_.end(), k, [](const value_type& a, const K& b) { return a.first < b; }); }
    const_iterator lower_bound(const K& k) const { return std::lower_bound(v_.begin(), v_.end(), k, [](const value_type& a, const K& b) { return a.first < b; }); }
    iterator upper_bound(const K& k) { return std::upper_bound(v_.begin(), v_.end(), k, [](const K& a, const value_type& b) { return a < b.first; }); }
    const_iterator upper_bound(const K& k) const { return std::upper_bound(v_.begin(), v_.end(), k, [](const K& a, const value_type& b) { return a < b.first; }); }
    iterator find(const K& k) { iterator it = lower_bound(k); return it != v_.end() && it->first == k ? it : v_.end(); }
    const_iterator find(const K& k) const { const_iterator it = lower_bound(k); return it != v_.end() && it->first == k ? it : v_.end(); }
    size_t count(const K& k) const { return find(k) != v_.end() ? 1 : 0; }
    V& operator[](const K& k) {
        if (v_.empty() || v_.back().first < k) { v_.emplace_back(k, V()); return v_.back().second; }
        iterator it = lower_bound(k);
        if (it != v_.end() && it->first == k) return it->second;
        return v_.insert(it, value_type(k, V()))->second;
    }
    V& at(const K& k) { iterator it = find(k); if (it == v_.end()) throw std::out_of_range("FlatMap::at"); return it->second; }
    const V& at(const K& k) const { const_iterator it = find(k); if (it == v_.end()) throw std::out_of_range("FlatMap::at"); return it->second; }
    iterator erase(iterator it) { return v_.erase(it); }
    size_t erase(const K& k) { iterator it = find(k); if (it == v_.end()) return 0; v_.erase(it); return 1; }
private:
    std::vector<value_type> v_;
};

// types_structs.rs:68-85 (the fields the hot path reads); ordered (flat) maps: positions ascend
struct Frag {
    std::string id;
    size_t counter_id = 0;
    FlatMap<SnpPosition, Genotype> seq_dict;
    FlatMap<SnpPosition, uint8_t> qual_dict;
    SnpPosition first_position = UINT32_MAX, last_position = 0;
    // the fields ingest fills for the writers (types_structs.rs:80-84)
    bool is_paired = false;
    bool merged_positions = false;                                       // `positions` was extended by a mate's / supplementary piece's set (file_reader.rs:541, 639): its iteration order is not that of one CIGAR walk
    GnPosition first_pos_base = SIZE_MAX, last_pos_base = SIZE_MAX;      // reference span of the alignment (0-based start, end exclusive)
    size_t seq_len[2] = {0, 0};                                          // bases of seq_string[0], seq_string[1]
    std::string seq_string[2];                                           // only kept with --output-reads: DnaString::from_acgt_bytes of SEQ (anything but ACGT -> A)
    std::vector<uint8_t> qual_string[2];                                 // QUAL + 33
    FlatMap<SnpPosition, std::pair<uint8_t, GnPosition>> snp_pos_to_seq_pos;
    // What `positions` (types_structs.rs:79, the FxHashSet the reference's distance loop iterates, utils_frags.rs:35) went through, kept only where it is NOT the
    // set of one CIGAR walk: the SNP positions of every alignment combine_frags merged into this fragment, in merge order (positions.extend(..), file_reader.rs:541
    // and :639; segment 0 = the receiving alignment, possibly empty), and the positions --ignore-monomorphic removed afterwards (utils_frags.rs:745-755).
    // positions_order() replays that on an emulated set; a Batch hands the result to the library as floria_pileup_packed::set_order for the reference-arithmetic mode.
    std::vector<std::vector<SnpPosition>> position_segments;
    std::vector<SnpPosition> removed_positions;
    bool other_set_order() const { return !position_segments.empty() || !removed_positions.empty(); }
    std::vector<SnpPosition> positions_order() const;                    // the positions in the iteration order of the set
    void update(SnpPosition snp_pos, Genotype geno, uint8_t qual) {      // update_frag, types_structs.rs:286-324
        seq_dict[snp_pos] = geno; qual_dict[snp_pos] = qual;
        if (snp_pos < first_position) first_position = snp_pos;
        if (snp_pos > last_position) last_position = snp_pos;
    }
    bool operator<(const Frag& o) const {                                 // Frag::cmp, types_structs.rs:87-93
        if (first_position != o.first_position) return first_position < o.first_position;
        if (last_position != o.last_position) return last_position > o.last_position;
        return counter_id < o.counter_id;
    }
};

// types_structs.rs:155-166
struct HapNode {
    std::vector<const Frag*> frag_set;                                   // ascending counter_id
    std::vector<std::pair<size_t, double>> out_edges, in_edges, out_flows;
    size_t column = SIZE_MAX, row = SIZE_MAX, id = SIZE_MAX;
    double cov = 0.0;
    std::pair<SnpPosition, SnpPosition> snp_endpoints;
    uint32_t block = 0;                                                  // the block of the S1 call the column was made from (its index in that call)
};

// One context + the contig currently resident in HBM.
class Session {
public:
    explicit Session(int device = 0);
    ~Session();
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    floria_hip_ctx* ctx() const { return ctx_; }
    // flatten + upload `all_frags` (must be sorted by Frag::cmp with counter_id == index, floria.rs:289-293)
    void load_contig(const std::vector<Frag>& all_frags);
    floria_hip_contig* contig() const { return contig_; }
    const std::vector<Frag>* frags() const { return frags_; }
private:
    floria_hip_ctx* ctx_ = nullptr;
    floria_hip_contig* contig_ = nullptr;
    const std::vector<Frag>* frags_ = nullptr;
};

// Contigs -> devices of one node: longest-processing-time-first on an estimated cost (the rule of floria_amd/shard.py, which bench.py broadcasts over
// RCCL): items in descending cost (ties: ascending index) go to the least loaded device (ties: the lowest).  Contigs share nothing, so the node-level
// parallelism of the reference (one rayon pool over the blocks of a contig, graph_processing.rs:345-362) becomes contigs dealt to GPUs.
std::vector<uint32_t> lpt_assign(const std::vector<double>& costs, uint32_t world);

std::vector<std::pair<SnpPosition, SnpPosition>> get_range_with_lengths(const std::vector<GnPosition>& snp_to_genome_pos, size_t block_length,
                                                                          size_t overlap_len, double minimal_density);

// graph_processing.rs:325-372.  `floria_out_dir` is only used by the reference's --debug dumps and is ignored here.
std::vector<std::vector<HapNode>> generate_hap_graph(Session& s, const std::vector<Frag>& all_frags, const std::vector<GnPosition>& snp_to_genome_pos,
                                                     const std::string& floria_out_dir, const Options& options);

// part_block_manip.rs:174-274.  Reads are visited in ascending counter_id unless `visit_order` (counter_ids) is given
// (the reference follows its FxHashMap's iteration order).
std::pair<std::vector<std::vector<const Frag*>>, std::vector<std::pair<SnpPosition, SnpPosition>>> process_reads_for_final_parts(
    Session& s, const std::vector<std::vector<const Frag*>>& all_joined_path_parts, const std::vector<Frag>& short_frags,
    const std::vector<std::pair<SnpPosition, SnpPosition>>& snp_range_parts_vec, const Options& options, const std::vector<GnPosition>& snp_to_genome_pos,
    const std::vector<uint32_t>* visit_order = nullptr);

// solve_flow.rs: FlowUpVec = Vec<((column, row), (column, row), flow)>
struct FlowUpdate { std::pair<size_t, size_t> n1, n2; double flow; };
typedef std::vector<FlowUpdate> FlowUpVec;
// The LP's optimum is usually not unique (stitch.cpp).  LpTie picks which optimal vertex the flow solver returns (the two extremes of its
// tie-breaking); LpInfo reports the optimal value and how many edges carry a different flow in some other optimal solution.
enum class LpTie { First, Last };
struct LpInfo { int64_t cost = 0; size_t movable_edges = 0; };
FlowUpVec solve_lp_graph(const std::vector<std::vector<HapNode>>& hap_graph, LpTie tie = LpTie::First, LpInfo* info = nullptr);
// get_disjoint_paths_rewrite in two halves.  The peeling decides from node coordinates, block ranges and flows alone: per path its nodes (column, row), in the order the
// trace-back visits them (sink first), and the SNP range they span.  The union concatenates the frag_sets of a path's nodes, sorts by counter_id and drops repeats.
struct PeeledPath { std::vector<std::pair<size_t, size_t>> nodes; std::pair<SnpPosition, SnpPosition> ends; };
std::vector<PeeledPath> peel_disjoint_paths(std::vector<std::vector<HapNode>>& hap_graph, const FlowUpVec& flow_update_vec, const Options& options);
std::pair<std::vector<std::vector<const Frag*>>, std::vector<std::pair<SnpPosition, SnpPosition>>> unite_paths(const std::vector<std::vector<HapNode>>& hap_graph,
                                                                                                                 const std::vector<PeeledPath>& paths);
std::pair<std::vector<std::vector<const Frag*>>, std::vector<std::pair<SnpPosition, SnpPosition>>> get_disjoint_paths_rewrite(
    std::vector<std::vector<HapNode>>& hap_graph, const FlowUpVec& flow_update_vec, const Options& options);
std::vector<const Frag*> get_frags_in_snpless_gaps(const std::vector<std::pair<SnpPosition, SnpPosition>>& path_parts, const std::vector<GnPosition>& snp_to_gn_pos,
                                                   const std::vector<Frag>& snpless_frags, GnPosition block_len, const std::vector<Frag>& final_frags);

// file_writer.rs:21-84.  `out_bam_part_dir` is the contig's output directory (its path is part of every HAP header), `options.out_dir`
// holds contig_ploidy_info.tsv (appended to; the header is written by write_run_files).  --output-reads (fastq) is not supported.
void write_outputs(Session& s, const std::vector<std::vector<const Frag*>>& part, const std::vector<std::pair<SnpPosition, SnpPosition>>& snp_range_parts_vec,
                   const std::string& out_bam_part_dir, const std::string& prefix, const std::string& contig, const std::vector<GnPosition>& snp_pos_to_genome_pos,
                   const Options& options, const std::vector<const Frag*>& snpless_frags, size_t contig_len);
// parse_cmd_line.rs:116-135: create the output directory (it must not exist unless --overwrite), cmd.log, contig_ploidy_info.tsv header
void prepare_contig_dir(const std::string& contig_out_dir, const Options& options);       // --overwrite: remove_dir_all of an existing contig directory (floria.rs:271-281)
void write_run_files(const Options& options, int argc, char** argv, const std::string& note = std::string());    // note: a second line of cmd.log

// ---- ingest (file_reader.rs) ---------------------------------------------------------------------------------------------------
struct VcfProfile {          // types_structs.rs:53-58, per contig; plus get_genotypes_from_vcf_hts' position vectors (:113-175)
    std::map<std::string, std::map<GnPosition, std::vector<Genotype>>> vcf_pos_allele_map;
    std::map<std::string, std::map<GnPosition, SnpPosition>> vcf_pos_to_snp_counter_map;
    std::map<std::string, std::map<SnpPosition, GnPosition>> vcf_snp_pos_to_gn_pos_map;
    std::map<std::string, std::vector<GnPosition>> snp_to_genome_pos;
};
// A record is a set of views into the inflated BAM stream the BamFile keeps alive: nothing is copied or unpacked per record
// (200 k long reads = 2 GB of bases; a per-record std::string each made the parallel decode slower than the serial one).
struct BamSeqView {                    // SEQ, 4 bits per base
    const unsigned char* packed = nullptr; size_t n = 0;
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    char operator[](size_t k) const { const unsigned char b = packed[k >> 1]; return "=ACMGRSVTWYHKDBN"[(k & 1) ? (b & 15) : (b >> 4)]; }
};
struct BamBytesView {                  // QUAL
    const uint8_t* p = nullptr; size_t n = 0;
    size_t size() const { return n; }
    uint8_t operator[](size_t k) const { return p[k]; }
};
struct BamCigarView {                  // n x u32 (len << 4 | op), possibly unaligned
    const unsigned char* p = nullptr; size_t n = 0;
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    uint32_t operator[](size_t k) const { uint32_t v; memcpy(&v, p + 4 * k, 4); return v; }
};
struct BamRecord {
    int32_t tid = -1, pos = 0;
    uint8_t mapq = 0;
    uint16_t flags = 0;
    std::string_view qname;
    BamCigarView cigar;
    BamSeqView seq;                    // ASCII bases through operator[]
    BamBytesView qual;
};
// --inflate device: what a segment owns when its records lie on the device.  The inflated members are a blob there, the records' header fields and names came back as a
// table (floria_hip_blob_records_opt).  The views of such a segment's records hold BLOB OFFSETS in their pointers (cigar.p, seq.packed, qual.p: byte offsets from a null
// base, as the header comment of floria_hip_blob_records derives them; never dereferenced on the host) and their qnames point into the table's names.
struct DeviceSegment {
    floria_hip_ctx* ctx = nullptr;
    floria_hip_blob* blob = nullptr;
    floria_blob_records* table = nullptr;
    std::vector<uint64_t> rec_off, rec_end;            // per record of the segment: its block_size prefix and the byte behind it, in the blob
    mutable uint64_t bytes_down = 0;                   // record bytes that came down for the host's use (CG-tag records, host-walk contigs)
    DeviceSegment() = default;
    DeviceSegment(const DeviceSegment&) = delete;
    DeviceSegment& operator=(const DeviceSegment&) = delete;
    ~DeviceSegment() { floria_hip_blob_records_free(table); floria_hip_blob_free(blob); }
};
struct BamFile {
    std::vector<unsigned char> raw;    // the inflated stream (the records point into it: a BamFile may be moved, not copied); empty for a device segment
    std::unique_ptr<DeviceSegment> dev;    // --inflate device: the segment's blob and record table (see DeviceSegment)
    std::vector<std::string> target_names;
    std::vector<uint64_t> target_len;
    std::vector<BamRecord> records;    // file order
    std::vector<std::vector<uint32_t>> by_tid;     // record indices per target, file order (what an indexed fetch() of the contig yields)
    int32_t tid_begin = 0, tid_end = 0;            // BamStream segments: the targets [tid_begin, tid_end) are COMPLETE in this segment (read_bam: all of them)
    BamFile() = default;
    BamFile(BamFile&&) = default;
    BamFile& operator=(BamFile&&) = default;
    BamFile(const BamFile&) = delete;
    BamFile& operator=(const BamFile&) = delete;
};
// The .bai index of a BAM (SAM specification 5.2), as far as a per-target seek needs it: for every target the virtual offset (coffset << 16 | uoffset) of its
// first record, the smallest chunk begin over its real bins, and that of the end of its last one (the largest chunk end: a hint, the records decide).  A target
// without a bin has no record.  The metadata pseudo-bin 37450 may be absent; where present its ref_beg must equal the smallest chunk begin.  Every length is checked
// against the file: a truncated or malformed index is FLORIA_E_INVALID naming the index file.  CSI is not read.
struct BaiIndex {
    struct Target { bool has_records = false; uint64_t begin = 0, end = 0; };
    std::string path;
    std::vector<Target> targets;
    uint64_t n_no_coor = 0;
    bool has_n_no_coor = false;
};
BaiIndex read_bai(const std::string& path);
std::string find_bai(const std::string& bam_path);         // X.bam.bai, then X.bai; "" when neither exists
// A coordinate-sorted BAM in bounded memory: the file is mapped, its BGZF members are indexed from their headers (no inflation), and next() inflates
// (in parallel) just enough members to return the records of the next run of COMPLETE targets — at least `min_bytes` of inflated records, more only when one
// target alone is larger.  A file that is not sorted by target is refused, a gzip file without BGZF members is read whole (one segment).
// Without an index every member is inflated in file order: targets come in header order in a sorted file.  With `use_index` and a .bai beside the file (find_bai)
// the member headers are walked lazily and select() narrows next() to the targets named: each is read from the offset the index gives for it up to the first
// record of another target, as the reference fetches one contig at a time (file_reader.rs:389-436); a target without a bin costs nothing.  Segments stay runs of
// complete targets [tid_begin, tid_end) in header order, the unselected ones among them without records.  Before select() (the parameter estimate) and without
// an index the stream reads the file from its start, segment by segment, as it always has.
class BamStream {
public:
    BamStream(const std::string& path, size_t threads = 1, bool use_index = false);
    ~BamStream();
    BamStream(const BamStream&) = delete;
    BamStream& operator=(const BamStream&) = delete;
    const std::vector<std::string>& target_names() const;
    bool next(BamFile& segment, size_t min_bytes);     // false: end of file (every target has been handed out)
    void rewind();
    size_t peak_buffer_bytes() const;                  // largest inflated buffer so far (what "bounded" means for this file)
    // Only these targets from here on (once, at the start of a pass).  Without an index the call changes nothing: every record is still handed out.
    void select(const std::vector<int32_t>& tids);
    const std::string& index_path() const;             // "" when no index is in use
    struct IndexUse { size_t selected, members_inflated, members_in_file; };
    IndexUse index_use() const;                        // (members_in_file walks the member headers that have not been walked yet)
    // --inflate device: from here on (after the parameter estimate's pass and its rewind(); under --estimate device also in front of that pass, which then reads the
    // unindexed segments described below, and again behind its rewind()) next() inflates nothing on the host.  Each call begins at the first record.  It plans a run of ADJACENT
    // members of the mapped file and the chains to walk in it, has them inflated on the context (floria_hip_inflate_bgzf uploads everything between the first and the
    // last member, so a segment never spans a gap between selected targets) and reads the record table (floria_hip_blob_records_opt): the segment it hands out is a
    // BamFile with `dev` and without `raw`.  With an index: one ONE_REF | CUT_TAIL chain per selected target from the index's offset, members up to the index's end
    // offset plus look-ahead, re-planned with twice the look-ahead where a chain meets the blob's end before another target.  Without: members in file order until
    // their ISIZEs sum to the window, one CUT_TAIL chain; the targets below the last record's are complete and the next segment begins at the member that holds the
    // first record of the incomplete one (those members are inflated again: the blob stays one buffer).  A gzip file without BGZF members is refused.
    void inflate_on_device(floria_hip_ctx* ctx);
    struct DeviceUse {                                 // members and bytes are totals SENT: a segment re-planned for look-ahead and carried-over members count again
        size_t segments = 0, members = 0, replanned = 0, carried_members = 0;
        uint64_t compressed_bytes = 0, inflated_bytes = 0, cg_bytes_down = 0;
        double inflate_s = 0., table_s = 0.;
    };
    DeviceUse device_use() const;
private:
    struct Impl;
    std::unique_ptr<Impl> p_;
};
BamFile read_bam(const std::string& path, size_t threads = 1);                         // BGZF + BAM, whole file (no index needed); members and records decode in parallel
std::vector<std::string> get_contigs_to_phase(const BamFile& bam);                     // file_reader.rs:738-746
VcfProfile get_vcf_profile(const std::string& vcf_file, const std::vector<std::string>& ref_chroms);       // :239-314 (+ :113-175); text VCF, optionally gzipped
std::map<std::string, std::string> get_fasta_seqs(const std::string& fasta_file);      // :462-489 (whole sequences)
// :343-460 + combine_frags :491-659 + frag_from_record :661-736; with `ref_seq` (the contig's reference sequence) every call is
// realigned (alignment.rs:7-64, exact affine-gap DP in place of block-aligner; options.realign_walk: a selected fixed-block walk)
std::pair<std::vector<Frag>, std::vector<Frag>> get_frags_from_bamvcf_rewrite(const BamFile& bam, const VcfProfile& vcf_profile, const Options& options, const std::string& contig,
                                                                               const std::string* ref_seq = nullptr);
// The same in two halves with the realignment's DP on the device between them.  alignment::realign decides most calls from the mismatch
// count of the two 32-base windows (an exact shortcut); the windows it cannot decide are queued — read window, reference window,
// candidate alleles, and the place the winning allele goes — scored by floria_hip_realign for a whole batch of contigs at once
// (Session::realign), and only then are mates and supplementary pieces merged (combine_frags copies the calls).
struct RealignQueue {
    std::vector<uint8_t> read_windows, ref_windows, alleles, n_alleles;    // 32 / 32 / FLORIA_MAX_ALLELES / 1 bytes per call
    std::vector<Genotype*> dst;
    size_t size() const { return dst.size(); }
    void append(RealignQueue&& other);
};
// The CIGAR walks of one ingest round in ONE device call, whichever route makes it (--pileup device / fused: RecordPileup, resident: ResidentPileup).  Every record of
// the given contigs that passes alignment_passed_check is sent as offsets into the segment's inflated buffer (the stretch of bam.raw that holds those records travels
// as it is).  A contig whose SNP counters are not rank + 1 in position order (a VCF that repeats a position) or that has a site with more than FLORIA_MAX_ALLELES
// alleles is not sent: its records keep the host walk (host_contigs names them).
struct RecordSelection;                                      // what floria_hip_pileup_records* takes (ingest.cpp)
class RoundWalk {
public:
    size_t records_sent = 0, blob_bytes = 0;
    double kernel_ms = 0., h2d_ms = 0., d2h_ms = 0.;         // floria_hip_last_timing of the call
    std::vector<std::string> host_contigs;
    floria_realign_counts counts = {};                       // of a realigning call
protected:
    RoundWalk() = default;
    // selects the round's records (ref_seqs: with the contigs' reference sequences) and, where there are any, makes the route's one device call (`call` throws when
    // it fails) and keeps its event times and the records' places in it.  Called by the route's constructor.
    void walk(Session& s, const BamFile& bam, const VcfProfile& vcf_profile, const Options& options, const std::string* contigs, size_t n_contigs,
              const std::map<std::string, std::string>* ref_seqs, const std::function<void(const RecordSelection&)>& call);
    std::vector<uint32_t> slot_;                             // record index of the segment -> position in the call + 1 (0: not sent)
    std::vector<int32_t> table_of_;                          // contig of the list -> contig of the call's SNP table, -1
    std::vector<uint64_t> snp_count_;                        // per table contig
};
// --pileup device: floria_hip_pileup_records.  A ContigIngest given the result fills its Frags from the records' cells instead of walking their CIGARs.
class RecordPileup : public RoundWalk {
public:
    // ref_seqs (--pileup fused): the reference sequences by contig name; the call is then floria_hip_pileup_records_realign with options.realign_walk / walk, the cells come
    // back realigned (a contig that is not in the map travels with an empty sequence: its cells stay as walked) and `realigned` tells ContigIngest to leave them alone
    RecordPileup(Session& s, const BamFile& bam, const VcfProfile& vcf_profile, const Options& options, const std::string* contigs, size_t n_contigs,
                 const std::map<std::string, std::string>* ref_seqs = nullptr);
    ~RecordPileup();
    RecordPileup(const RecordPileup&) = delete;
    RecordPileup& operator=(const RecordPileup&) = delete;
    struct Cells { const uint32_t* snp; const uint8_t* allele; const uint8_t* qual; const uint32_t* seq_pos; size_t n; int64_t ref_end; };
    bool cells(uint32_t record_index, Cells& out) const;     // false: the record was not sent
    bool realigned = false;
private:
    floria_record_cells* cells_ = nullptr;
};
struct ContigPlan;
class ContigIngest {
public:
    // records of `contig` -> one Frag per passing alignment (file_reader.rs:343-430); with a queue the undecided realignments are deferred; with a RecordPileup the
    // records it holds are not walked (and not realigned here when it holds realigned cells)
    ContigIngest(const BamFile& bam, const VcfProfile& vcf_profile, const Options& options, const std::string& contig, const std::string* ref_seq, RealignQueue* queue,
                 const RecordPileup* device_cells = nullptr);
    ~ContigIngest();
    ContigIngest(ContigIngest&&) noexcept;
    ContigIngest& operator=(ContigIngest&&) noexcept;
    // combine_frags (:491-659) -> (frags with SNPs in Frag::cmp order, frags without): plan() decides who is merged onto whom, the Frags are merged in its order
    std::pair<std::vector<Frag>, std::vector<Frag>> finish();
    ContigPlan plan() const;                                      // the fragment plan of the records held (before finish()): also --dump-plan under the routes that walk into Frags
private:
    struct Impl;
    std::unique_ptr<Impl> p_;
};

// ---- --pileup resident: fragments planned from headers ------------------------------------------------------------------------------------
// What combine_frags (file_reader.rs:491-659) reads of one passing alignment when it decides who is merged onto whom: its flags, its place among the contig's records
// (Frag::counter_id before the sort) and the first / last SNP of its walk.  The host walk has them in its Frags, floria_hip_pileup_records_resident returns them in
// its summary; no cell is needed.
struct PlanRecord {
    uint32_t rec = 0;                                    // index into BamFile::records of the segment
    uint16_t flags = 0;
    size_t counter_id = 0;
    SnpPosition first = UINT32_MAX, last = 0;            // Frag::first_position / last_position of the walk; UINT32_MAX / 0: the record has no cell
    bool has_cells() const { return first != UINT32_MAX; }
};
struct PlannedFrag {
    std::vector<PlanRecord> parts;                       // merge order: the first is the base, each later one is `extend`ed onto it
    std::vector<uint8_t> mate;                           // per part: 1 for the second mate's part (file_reader.rs:556-562)
    SnpPosition first = UINT32_MAX, last = 0;            // of the merged fragment
    size_t counter_id = 0;                               // the base's
};
struct ContigPlan {
    std::vector<PlannedFrag> frags;                      // sorted by Frag::cmp: the pileup's read order
    std::vector<PlannedFrag> snpless;                    // fragments whose parts hold no cell, in the order combine_frags yields them
};
// combine_frags on headers: `groups` = the passing records of every read name, in record order, names in the order of their first record; snp_to_gn as
// VcfProfile::vcf_snp_pos_to_gn_pos_map of the contig.  A two-record paired group: sorted by (flags, Frag::cmp), flag 64 first -> (first, second), flag 128 first ->
// (second, first), the extension marked as mate 1.  A lone primary record passes.  Anything else: no primary -> dropped; a gap of more than supp_aln_dist_cutoff bases
// between consecutive sorted (first, last) intervals of the parts with cells -> the LAST primary alone; otherwise that primary, then every other part in record order.
ContigPlan plan_contig(std::vector<std::vector<PlanRecord>>& groups, const std::map<SnpPosition, GnPosition>& snp_to_gn, int64_t supp_aln_dist_cutoff);
// --dump-plan: "#CONTIG name n_frags n_snpless", then per fragment "F id first last part .." and per snpless fragment "S id part ..", a part as name:flag:pos:mate
std::string plan_text(const std::string& contig, const ContigPlan& plan, const BamFile& bam);

struct ContigHandle {                                    // an owned floria_hip_contig (freed on the thread that lets go of it: one host thread at a time per context)
    floria_hip_contig* h = nullptr;
    ContigHandle() = default;
    explicit ContigHandle(floria_hip_contig* p) : h(p) {}
    ContigHandle(ContigHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    ContigHandle& operator=(ContigHandle&& o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ContigHandle(const ContigHandle&) = delete;
    ContigHandle& operator=(const ContigHandle&) = delete;
    ~ContigHandle() { reset(); }
    void reset(floria_hip_contig* p = nullptr) { if (h) floria_hip_contig_free(h); h = p; }
    floria_hip_contig* get() const { return h; }
    explicit operator bool() const { return h != nullptr; }
};
// One contig of a resident round: header-only Frags (id, first / last position, first / last base, is_paired, sequences with --output-reads; NO seq_dict, qual_dict,
// positions or snp_pos_to_seq_pos), the plan they came from, and after ResidentPileup::assemble the handle of the contig on the device.
struct HeaderContig {
    ContigPlan plan;
    std::vector<Frag> all_frags, frags_without_snps;     // all_frags in plan order with counter_id == index
    uint64_t part_cells = 0;                             // cells of all parts of all_frags (from cell_off): an upper bound of the merged count
    size_t merged_frags = 0;                             // fragments with two or more parts that have cells
    ContigHandle handle;
};
// The walks of one ingest round in ONE floria_hip_pileup_records_resident call (RecordPileup's record selection and host_contigs rule; with ref_seqs the calls are
// realigned there, options.realign_walk / walk honoured), then per contig a plan from the summary, one floria_hip_assemble_contigs_opt call for the round and, with
// --ignore-monomorphic, one floria_hip_drop_monomorphic call.  assemble() must run before the context's next floria_hip_pileup_records* call (include/floria_hip.h, RESIDENCY).
class ResidentPileup : public RoundWalk {
public:
    ResidentPileup(Session& s, const BamFile& bam, const VcfProfile& vcf_profile, const Options& options, const std::string* contigs, size_t n_contigs,
                   const std::map<std::string, std::string>* ref_seqs = nullptr);
    ~ResidentPileup();
    ResidentPileup(const ResidentPileup&) = delete;
    ResidentPileup& operator=(const ResidentPileup&) = delete;
    bool on_table(size_t contig_index) const { return table_of_[contig_index] >= 0; }      // false: the contig keeps the host walk (or is unknown to the BAM / VCF)
    HeaderContig plan(size_t contig_index) const;                                          // thread-safe: reads the summary
    // planned[i] (may be null where !on_table(i)) for every contig of the constructor's list; fills planned[i]->handle and re-maps the Frags through the filter
    void assemble(std::vector<HeaderContig*>& planned, bool derive_set_order, bool keep_seq_pos, bool ignore_monomorphic, double epsilon);
    double assemble_s = 0., filter_s = 0.;                   // wall seconds of the assemble and the filter call
    double sequences_s = 0.;                                 // device segment, --output-reads: wall seconds of the round's floria_hip_blob_sequences call
    double assemble_ms = 0., filter_ms = 0.;                 // their device-event totals
    uint64_t bytes_back = 0;                                 // what the host received: the summary's arrays, the filter's three words per read, its mask and map
    uint64_t removed_snps = 0, dropped_reads = 0;            // --ignore-monomorphic
private:
    Session& s_;
    const BamFile& bam_;
    const VcfProfile& vp_;
    const Options& o_;
    const std::string* contigs_;
    floria_record_summary* summary_ = nullptr;
    void fetch_sequences(std::vector<HeaderContig*>& planned);   // device segment: the kept sequences of every planned fragment in one floria_hip_blob_sequences call
};
// --inflate device: the records of one target of a device segment as a host BamFile (the bytes of its chain in one floria_hip_blob_download, decoded as a host
// segment's are) for a contig that keeps the host walk; counts the bytes into segment.dev->bytes_down
BamFile host_copy_of_target(const BamFile& segment, const std::string& contig, size_t threads);
std::pair<size_t, double> l_epsilon_auto_detect(const BamFile& bam);                   // :749-826
// The same fed segment by segment (complete targets in header order, as BamStream::next yields them): done() once 1000 columns have been sampled,
// which is where the reference's pileup loop breaks as well.
class EpsilonEstimator {
public:
    EpsilonEstimator();
    ~EpsilonEstimator();
    void feed(const BamFile& segment);
    // The same for a device segment (--estimate device): the records are filtered on the segment's table, grouped by target and handed to one
    // floria_hip_blob_estimate call with the state carried so far; the sampled columns and the records' hits that come back go through the combine step below.
    void feed_device(const BamFile& segment);
    // The combine step both routes end in: a sampled column (with total >= 5 it gives one more error rate), and `hits` more entries of l_seq in the length multiset.
    void add_column(int32_t tid, int32_t pos, uint32_t total, uint32_t most);
    void add_length(size_t l_seq, uint64_t hits);
    bool done() const;
    std::pair<size_t, double> result();                // (block length, epsilon)
    // --dump-estimate: "tid pos total most" per sampled column, then "count N", "n_err N" and one "length L M" per distinct l_seq, ascending
    void dump(std::ostream& out) const;
    size_t device_calls = 0;                           // feed_device: calls, and their device events (floria_hip_last_timing)
    double device_kernel_ms = 0., device_h2d_ms = 0., device_d2h_ms = 0.;
private:
    struct Impl;
    std::unique_ptr<Impl> p_;
};

// part_block_manip.rs:517-616: (hapqs, rel_err per haploset, avg_err) — the HAPQ / REL_ERR header fields and the contig table's avg_err.
struct HapqResult { std::vector<uint8_t> hapqs; std::vector<double> rel_err; double avg_err = 0.0; };

// ---- many contigs at once ---------------------------------------------------------------------------------------------------------------
// The reference walks its contigs serially (floria.rs:229) because its parallelism is inside a contig (rayon over blocks).  On the
// GPU the throughput comes from thousands of blocks in flight, and a metagenome has thousands of small contigs: a host takes a batch
// of contigs through every stage together — one pipelined upload + S1 call, one hap-graph call, the LP / path peeling per contig
// on host threads, one S2 call, one COV/ERR and one HAPQ call — and writes the files contig by contig.  Results per contig are
// exactly those of the per-contig functions above.
struct ContigWork {
    std::string name, out_dir;
    std::vector<Frag> all_frags, frags_without_snps;                   // all_frags sorted, counter_id == index (floria.rs:289-293)
    const std::vector<GnPosition>* snp_to_genome_pos = nullptr;
    size_t contig_len = 0;
    // filled stage by stage
    std::vector<std::pair<SnpPosition, SnpPosition>> iter_vec;         // get_range_with_lengths
    std::vector<std::vector<HapNode>> hap_graph;                       // generate_hap_graph
    FlowUpVec flows;                                                   // solve_lp_graph
    std::vector<std::vector<const Frag*>> path_parts, final_parts;     // get_disjoint_paths_rewrite / process_reads_for_final_parts
    std::vector<std::pair<SnpPosition, SnpPosition>> path_ranges, final_ranges;
    std::vector<PeeledPath> path_nodes;                                // --paths resident: peel_disjoint_paths (path_parts then stay empty unless --debug)
    std::vector<const Frag*> snpless;                                  // get_frags_in_snpless_gaps
    std::vector<double> stats;                                         // 4 per final haploset: cov, err, total_err, total_cov
    HapqResult hq;
    // --pileup resident: the contig as assembled on the device (all_frags then are header-only, ResidentPileup).  Owned here; whoever hands the ContigWork to another
    // thread resets it first (a context takes one host thread at a time).
    ContigHandle handle;
    uint64_t resident_cells = 0;                                       // cells of the parts of its fragments (floria_record_summary::cell_off): what --batch-cells counts for it
    // ... and what the writers would have read in the cells, filled by Batch::stats_and_hapq for a contig with a handle:
    std::vector<uint64_t> allele_off;                                  // [final haplosets + 1] positions before haploset k (its range length; 0 for an empty haploset)
    std::vector<uint32_t> allele_counts;                               // [4 * allele_off.back()] floria_hip_haploset_alleles: set_to_seq_dict(.., false) over the range
    std::vector<std::vector<uint32_t>> span_left, span_right;          // --output-reads: floria_hip_read_spans per final haploset, per read in final_parts[k] order
};
class Batch {
public:
    // marshals the Frags into the pinned compact wire form (floria_pileup_packed); with_set_orders: contigs that hold merged or cut-down fragments also get
    // the iteration orders of their fragments' position sets (set_order: what the reference-arithmetic mode needs to add in the reference's order)
    Batch(Session& s, std::vector<ContigWork>& work, bool with_set_orders = false);
    ~Batch();
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;
    void generate_hap_graphs(const Options& options);                  // upload + S1 + hap graph for every contig (graph_processing.rs:325-372)
    void process_reads_for_final_parts(const Options& options);        // S2 for every contig, from path_parts / path_ranges (--paths resident: from path_nodes, joined on the device)
    void stats_and_hapq(const Options& options);                       // get_errors_cov_from_frags + get_hapq for every final haploset; for contigs with a handle also the
                                                                       // writers' allele tables and, with --output-reads, their trim lookups
    // --dump-handles (tests): per contig "#CONTIG name n_reads", "#IDS id ..", then "#FIELD k v .." for floria_hip_contig_download fields 0-6 as uint32 words and
    // field 7 where the contig carries a set order; valid once generate_hap_graphs has run (every contig then has a handle, whichever route made it)
    std::string dump_handles() const;
    uint64_t bytes_back = 0;                                           // bytes of the allele tables and trim lookups received
    uint64_t paths_joined = 0;                                         // --paths resident: paths united on the device
    uint64_t haplosets_by_handle = 0;                                  // --haplosets resident: final haplosets whose statistics were computed from the handle
private:
    Session& s_;
    std::vector<ContigWork>& work_;
    void* pinned_ = nullptr;
    std::vector<size_t> host_ix_;                                      // the contigs without a handle of their own: marshalled here, piles_[j] is contig host_ix_[j]
    std::vector<floria_pileup_packed> piles_;
    std::vector<floria_hip_contig*> handles_;                          // per contig: the ContigWork's own handle, or the one uploaded here (owned_)
    floria_block_result* res_ = nullptr;                               // --paths resident: the S1 result (its batch stays resident) from generate_hap_graphs to the join
    floria_hip_haplosets* haplosets_ = nullptr;                        // --haplosets resident: S2's result on the device, from process_reads_for_final_parts to the destructor
    std::vector<char> owned_;
};
// utils_frags::remove_monomorphic_allele (utils_frags.rs:713-772, --ignore-monomorphic): SNPs where one allele carries (almost) all of the
// phred weight are dropped from every read; reads left without SNPs are dropped; the rest is sorted and renumbered
std::vector<Frag> remove_monomorphic_allele(std::vector<Frag> frags, double error);
// write_reads + write_nosnp_reads (file_writer.rs:86-150, 370-560, --output-reads): long_reads/{i}_part.fastq, short_reads/{i}_part_paired{1,2}.fastq, snpless*.fastq
// span_left / span_right (both or neither): floria_hip_read_spans' words per haploset and per read in part[i] order, for Frags that hold no snp_pos_to_seq_pos
void write_reads(const std::vector<std::vector<const Frag*>>& part, const std::vector<std::pair<SnpPosition, SnpPosition>>& snp_range_parts_vec, const std::string& out_bam_part_dir,
                 bool extend_read_clipping, const std::vector<uint8_t>& hapqs, bool gzip, const std::vector<std::vector<uint32_t>>* span_left = nullptr,
                 const std::vector<std::vector<uint32_t>>* span_right = nullptr);
void write_nosnp_reads(const std::string& out_bam_part_dir, const std::vector<const Frag*>& snpless_frags, bool gzip);
// scores the queued realignment windows on the device (floria_hip_realign; with a walk floria_hip_realign_walk) and stores the winning alleles where they belong
void realign_queue_on_device(Session& s, RealignQueue& queue, const floria_realign_walk* walk = nullptr);
// write_outputs for a contig whose statistics were computed by Batch::stats_and_hapq
void write_outputs(const ContigWork& w, const Options& options);
// the same in two halves, for hosts that write the contigs of a batch from several threads: the files of the contig (returns its
// contig_ploidy_info.tsv row), and the append of the rows in contig order
std::string write_contig_files(const ContigWork& w, const Options& options);
void append_contig_ploidy_row(const Options& options, const std::string& row);
HapqResult get_hapq(Session& s, const std::vector<std::vector<const Frag*>>& parts, const std::vector<GnPosition>& snp_to_genome_pos,
                    const std::vector<std::pair<SnpPosition, SnpPosition>>& snp_range_parts_vec, const Options& options);

}  // namespace floria
