/*
 * floria_hip.h — C ABI of libfloria_hip.so: the MI355X (gfx950) replacement for
 * floria's per-SNP-block read->haplotype clustering path.
 *
 * The reference (bluenote-1577/floria, Rust) has no FFI/plugin interface; this header cuts the
 * seam at the two Rust call sites a drop-in must satisfy:
 *
 *   S1  graph_processing.rs:345-362  the rayon par-for over blocks calling
 *       get_local_hap_blocks(all_frags, snp_to_genome_pos, dir, j, snp_range_vec, options)
 *       (graph_processing.rs:103-110)            -> floria_hip_phase_blocks()
 *   S2  floria.rs:359-366 calling part_block_manip::process_reads_for_final_parts(parts,
 *       short_frags, ranges, options, snp_to_gn) (part_block_manip.rs:174-180)
 *                                                -> floria_hip_reassign()
 *   plus utils_frags::get_range_with_lengths (utils_frags.rs:405-463), the host-side function
 *   that defines the work units (blocks)        -> floria_hip_block_ranges()
 *
 * Conventions
 *   - plain pointers and sizes only; every input is caller-owned and only read during the call;
 *   - outputs are library-owned and released with the matching *_free();
 *   - every entry point returns 0 on success, <0 on error (FLORIA_E_*); the message of the last
 *     error on the calling thread is floria_hip_last_error(); nothing throws across the ABI;
 *   - a context is bound to one device; one host thread at a time per context;
 *   - there is NO CPU fallback: if no gfx950 device / HIP runtime is usable, create() fails.
 *
 * SNP positions are floria's 1-based SNP indices (types_structs.rs:12 `SnpPosition = u32`),
 * reads are `Frag`s (types_structs.rs:68-85) flattened to CSR and sorted by `Frag::cmp`
 * (types_structs.rs:87-93: first_position asc, last_position desc, counter_id asc) with
 * counter_id == index (floria.rs:289-293).
 */
#ifndef FLORIA_HIP_H
#define FLORIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLORIA_OK            0
#define FLORIA_E_INVALID    -1   /* malformed argument / pileup violates an invariant            */
#define FLORIA_E_DEVICE     -2   /* HIP runtime / device error (message has the hipError string) */
#define FLORIA_E_NOMEM      -3   /* host or device allocation failed                             */
#define FLORIA_E_UNSUPPORTED -4  /* input outside the supported envelope (e.g. allele index > 3) */

#define FLORIA_MAX_ALLELES   4   /* 2-bit allele codes: 0 = ref, 1..3 = alt (file_reader.rs:702-710) */
#define FLORIA_MAX_PLOIDY    16

/* One contig's reads as a sparse reads x SNPs pileup (CSR).  Replaces `&Vec<Frag>`
 * (types_structs.rs:68-85): seq_dict -> (snp, allele), qual_dict -> qual, first/last_position.
 * Cells of a read are sorted by ascending snp; snp[read_off[r]] == first[r] and
 * snp[read_off[r+1]-1] == last[r]; every read has >= 1 cell. */
typedef struct {
    const uint32_t* read_off;  /* [n_reads+1] cell offsets                      */
    const uint32_t* snp;       /* [n_cells]   1-based SNP index of the cell     */
    const uint8_t*  allele;    /* [n_cells]   allele index 0..3                 */
    const uint8_t*  qual;      /* [n_cells]   base quality (phred, 0..255)      */
    const uint32_t* first;     /* [n_reads]   first_position                    */
    const uint32_t* last;      /* [n_reads]   last_position                     */
    uint32_t        n_reads;
    /* OPTIONAL (NULL = not given): the iteration order of every read's `positions` set — `for pos in r.positions.iter()`, utils_frags.rs:35 — for the
     * reference-arithmetic mode (floria_hip_set_option "arith" = 1), which adds a read's terms in that order.  set_order[read_off[r] + j] = index within
     * read r (0-based, in the ascending-SNP order of its cells) of the cell whose position the set yields j-th: a permutation of 0 .. L_r - 1 per read
     * (checked on the device; FLORIA_E_INVALID otherwise).  A Rust host writes it down while it marshals a Frag (it HAS the FxHashSet: whatever built it —
     * one CIGAR walk, `positions.extend(mate.positions)` of combine_frags, file_reader.rs:539-541 and :636-639, the removals of --ignore-monomorphic,
     * utils_frags.rs:745-755 — is in that order by construction).  With NULL the library emulates the set of ONE CIGAR walk (seq_dict.keys().collect(),
     * file_reader.rs:729-733; csrc/arith_kernel.h), which is what every fragment built from a single alignment has.  Ignored in arithmetic mode 0. */
    const uint32_t* set_order; /* [n_cells] or NULL */
} floria_pileup;

/* The same pileup in the compact wire form SURVEY.md §8(d) counts (per read: first, last; a presence bit per SNP of its span; a 2-bit
 * allele and one quality byte per observed SNP): 1.375 B per cell + 16 B per read instead of 6 B per cell + 12 B per read — what a
 * host marshals its `Vec<Frag>` into for the PCIe link (floria.rs:255-293); the device expands it to the CSR form above and then
 * validates + flattens that exactly as if it had been uploaded (upload_kernel.h: expand_kernel, flatten_kernel).
 *   present : read r owns bits [bit_off[r], bit_off[r+1]) with bit_off[r+1] - bit_off[r] == last[r] - first[r] + 1; bit j of the read
 *             (bit (bit_off[r]+j) & 7 of byte (bit_off[r]+j) >> 3, LSB first) is set iff SNP first[r] + j carries a call; the first and
 *             the last bit of a read are set and the number of set bits equals read_off[r+1] - read_off[r];
 *   allele2 : cell c (global cell index of the contig, as in read_off) at bits 2 (c & 3) of byte c >> 2; allele indices 0..3;
 *   qual    : one byte per cell. */
typedef struct {
    const uint32_t* read_off;  /* [n_reads+1] cell offsets                              */
    const uint32_t* first;     /* [n_reads]   first_position                            */
    const uint32_t* last;      /* [n_reads]   last_position                             */
    const uint32_t* bit_off;   /* [n_reads+1] offsets into `present`, in bits (< 2^32)  */
    const uint8_t*  present;   /* [ceil(bit_off[n_reads] / 8)]                          */
    const uint8_t*  allele2;   /* [ceil(n_cells / 4)]                                   */
    const uint8_t*  qual;      /* [n_cells]                                             */
    uint32_t        n_reads;
    const uint32_t* set_order; /* [n_cells] or NULL: as in floria_pileup (travels as it is, 4 B per cell, only when given) */
} floria_pileup_packed;

/* The fields of `Options` (types_structs.rs:20-51) the hot path reads
 * (graph_processing.rs:111-113,198-226,234). */
typedef struct {
    double   epsilon;             /* -e  */
    uint32_t max_ploidy;          /* -p  (default 5)  */
    uint32_t beam;                /* -n  max_number_solns (default 10) */
    uint32_t ploidy_sensitivity;  /* -s  1|2|3 (default 2) */
    int32_t  stopping_heuristic;  /* !--no-stop-heuristic (default 1) */
} floria_params;

/* Result of S1 for a batch of blocks (what get_local_hap_blocks returns, minus the HapNode
 * wrappers the host rebuilds with HapNode::new, types_structs.rs:169).  Block b has
 * n_b = read_off[b+1]-read_off[b] reads (0 <=> the reference returns None); read_id is ascending;
 * part[i] in [0,best_ploidy) is the partition (haplotype) of read_id[i] at the chosen ploidy;
 * mec[b*max_ploidy + p-1] is mec_vector[p-1] (graph_processing.rs:156-162), 0 for untried p. */
typedef struct {
    uint32_t  n_blocks;
    uint32_t  max_ploidy;
    uint32_t* best_ploidy;     /* [n_blocks]  0 if the block holds no reads */
    uint32_t* ploidies_tried;  /* [n_blocks]  last ploidy evaluated before the stop rule fired */
    uint64_t* read_off;        /* [n_blocks+1] */
    uint32_t* read_id;         /* [read_off[n_blocks]] */
    uint8_t*  part;            /* [read_off[n_blocks]] */
    double*   mec;             /* [n_blocks*max_ploidy] */
    double    min_prune_margin;/* min |p_k - lse - ln(PROB_CUTOFF)| over all pruning decisions
                                  (global_clustering.rs:98); parity certificate, see DESIGN.md */
    uint64_t  batch_token;     /* identifies the device-resident copy of this batch (floria_hip_hap_graph) */
} floria_block_result;

/* Hap-graph columns of the batch: HapNode::new's coverage statistic (types_structs.rs:179-193) for
 * every node (block b has best_ploidy[b] nodes) and update_hap_graph's out_weights (graph_processing.rs:28-47) for every
 * consecutive pair of non-empty blocks of a contig, BEFORE the >= MIN_SHARED_READS_UNAMBIG (2.0) filter of :51. */
typedef struct {
    uint32_t  n_blocks;
    uint64_t* node_off;        /* [n_blocks+1] */
    double*   node_cov;        /* [node_off[n_blocks]] */
    int32_t*  pred;            /* [n_blocks] previous non-empty block of the same contig, -1 if none */
    uint64_t* edge_off;        /* [n_blocks+1]; block b holds best_ploidy[pred[b]] x best_ploidy[b] counts, row-major */
    uint32_t* edge_w;          /* [edge_off[n_blocks]] */
} floria_hap_graph;

/* Haplogroups (S2 in/out): group g holds reads grp_read[grp_off[g]..grp_off[g+1]) and spans the
 * inclusive SNP range (range[2g], range[2g+1]).  Output groups are sorted by range
 * (part_block_manip.rs:276-288) and read ids ascend within a group. */
typedef struct {
    uint32_t  n_groups;
    uint64_t* grp_off;         /* [n_groups+1] */
    uint32_t* grp_read;        /* [grp_off[n_groups]] */
    uint32_t* range;           /* [2*n_groups] */
} floria_groups;

typedef struct {
    uint32_t  n;
    uint32_t* start;           /* [n] 1-based inclusive */
    uint32_t* end;             /* [n] 1-based inclusive */
} floria_ranges;

/* Per-kernel timing of the last phase_blocks / reassign call, measured with hipEvents on the
 * context's stream (bench.py's roofline leg reads this). */
typedef struct {
    double   beam_ms;          /* sum over launches of the beam-search kernel     */
    double   optimize_ms;      /* sum over launches of the optimise/MEC kernel    */
    double   select_ms;        /* stop-rule + gather kernels                      */
    double   reassign_ms;      /* S2 kernel                                       */
    double   h2d_ms, d2h_ms;   /* copies issued by the call                       */
    double   total_ms;         /* first launch -> last completion on the stream   */
    uint32_t beam_launches, optimize_launches;
    uint64_t algorithmic_bytes;/* SURVEY.md §8(d) bytes(block) summed over the call's blocks */
    uint64_t beam_steps;       /* reads consumed by beam search, summed over (block, ploidy) jobs */
    uint64_t beam_launch_bytes;/* sum over beam launches of bytes(block) of the blocks that launch phased */
    uint64_t jobs;             /* (block, ploidy) jobs actually run */
    uint32_t streams;          /* job groups of the last S1 call: their launch triples overlap on separate streams, so the
                                * per-kernel sums above can exceed phase_ms */
    uint32_t stage_width;      /* ploidies run concurrently per stage (1 = the reference's sequential ploidy loop, no speculative jobs) */
    double   phase_ms;         /* wall time of the per-ploidy launch loop (fork of the first group -> join of the last) */
    uint64_t upload_pinned_bytes; /* last upload: bytes that went by DMA straight from the caller's pinned memory */
    uint64_t upload_staged_bytes; /* last upload: bytes staged through the library's pinned ring (pageable sources)  */
    uint32_t upload_chunks;    /* floria_hip_phase_pileups_batch: chunks whose transfer overlapped the kernels (1 = not pipelined) */
    uint32_t optimize_packed_launches; /* optimise launches of the last S1 call that streamed the 4-byte packed cells ("opt_packed"); the others read the 8-byte cells */
    double   beam_union_ms;    /* wall time with at least one beam-search launch in flight (<= phase_ms; beam_ms, a sum over overlapping launches, can exceed it) */
    double   optimize_union_ms;/* ... with at least one optimise launch in flight */
    double   pileup_ms;        /* floria_hip_pileup_records: sum over the call's launches (count pass, offset scan, fill pass).  Appended with that entry point:
                                * floria_hip_last_timing writes the whole struct, so callers built against the shorter layout must be rebuilt */
    uint32_t optimize_delta_passes;    /* last S1 call, "opt_delta": distance passes behind an accepted round that exchanged only the terms at the flipped code bytes */
    uint32_t optimize_delta_fallbacks; /* ... that had flips and streamed the interval's reads instead (more flips than the list holds, or too many to pay).  Appended as pileup_ms was */
} floria_timing;

typedef struct floria_hip_ctx floria_hip_ctx;
typedef struct floria_hip_contig floria_hip_contig;   /* a pileup resident in HBM */

int  floria_hip_create(int device, floria_hip_ctx** out);
void floria_hip_destroy(floria_hip_ctx* ctx);
const char* floria_hip_last_error(void);
const char* floria_hip_version(void);
/* Step 0 for a host that links this library: call ONCE, from the main thread, BEFORE the process's first HIP call (floria_hip_create included).  It sets
 * GPU_MAX_HW_QUEUES=12 unless the variable is already set: HIP reads it once, when the runtime initialises, and maps streams onto that many hardware queues
 * (default 4); the job groups of S1, the upload pipeline and the speculative ploidy stages want their streams on separate queues.  Exporting the variable in the
 * process environment does the same.  Without it everything still works and returns the same results: floria_hip_create measures how many streams really run
 * side by side, keeps its launch plans within that and says so once on stderr (about 25 % less throughput from host memory).  The library itself never touches
 * the environment (setenv is not safe beside threads that read it). */
int  floria_hip_init_env(void);

/* utils_frags::get_range_with_lengths (utils_frags.rs:405-463), host side, exact restatement.
 * snp_to_genome_pos has n_snps entries (0-based SNP index -> bp).  Fails (FLORIA_E_INVALID) where
 * the reference exits (positions not increasing, utils_frags.rs:424-427). */
int  floria_hip_block_ranges(const uint64_t* snp_to_genome_pos, uint32_t n_snps,
                             uint64_t block_length, uint64_t overlap_len, double minimal_density,
                             floria_ranges** out);
void floria_hip_ranges_free(floria_ranges* r);

/* Upload one contig's pileup to HBM.  The invariants above are validated ON THE DEVICE while the pileup is flattened into
 * its resident form (allele | Q24 weight per cell, per-read hash constants and metadata records): the host touches no cell.
 * The handle can be phased any number of times. */
int  floria_hip_contig_upload(floria_hip_ctx* ctx, const floria_pileup* pileup, floria_hip_contig** out);
void floria_hip_contig_free(floria_hip_contig* c);

/* Upload n contigs in one go (what a host does once per batch of contigs it marshals from `Vec<Frag>`, floria.rs:255-293):
 * one device allocation, the raw arrays by DMA (arrays of consecutive contigs that are back to back in host memory travel as
 * ONE transfer; sources in floria_hip_host_alloc memory are not staged), one validate + flatten launch, one synchronisation.
 * out[0..n) receive the handles (each freed with floria_hip_contig_free); on error no handle is returned. */
int  floria_hip_contig_upload_batch(floria_hip_ctx* ctx, const floria_pileup* pileups, uint32_t n, floria_hip_contig** out);

/* Diagnostic: copy one resident array of a contig back to the host.  CELL_AW = allele << 28 | Q24 weight per cell
 * (phred_scale, utils_frags.rs:702-711), TW = the two per-read constants of the linear state hash, META = the packed per-read
 * record {cell offset, cell count, first, last, tw1 lo/hi, tw2 lo/hi}. */
#define FLORIA_FIELD_READ_OFF 0
#define FLORIA_FIELD_FIRST    1
#define FLORIA_FIELD_LAST     2
#define FLORIA_FIELD_SNP      3
#define FLORIA_FIELD_CELL_AW  4
#define FLORIA_FIELD_TW       5
#define FLORIA_FIELD_META     6
#define FLORIA_FIELD_SET_ORDER 7   /* uint32 [n_cells], only of a contig that carries a set_order (FLORIA_E_INVALID "the contig carries no set_order" otherwise) */
#define FLORIA_FIELD_SEQ_POS   8   /* uint32 [n_cells], the SEQ_POS words (floria_hip_assemble_contigs_opt), only of a contig that carries positions (FLORIA_E_INVALID "the contig carries no seq_pos (field 8 is an unknown field of a contig without positions)" otherwise) */
int  floria_hip_contig_download(const floria_hip_contig* c, int field, void* dst, size_t bytes);

/* Pinned host memory for pileup arrays (NULL on failure). */
void* floria_hip_host_alloc(size_t bytes);
void  floria_hip_host_free(void* p);

/* S1: phase n_blocks SNP ranges of one resident contig. */
int  floria_hip_phase_blocks_resident(floria_hip_ctx* ctx, const floria_hip_contig* contig,
                                      const uint32_t* blk_start, const uint32_t* blk_end,
                                      uint32_t n_blocks, const floria_params* params,
                                      floria_block_result** out);
/* S1 convenience: upload + phase + free. */
int  floria_hip_phase_blocks(floria_hip_ctx* ctx, const floria_pileup* pileup,
                             const uint32_t* blk_start, const uint32_t* blk_end, uint32_t n_blocks,
                             const floria_params* params, floria_block_result** out);
void floria_hip_block_result_free(floria_block_result* r);

/* S1 straight from HOST pileups for many contigs: upload_batch + phase_blocks_batch as one pipelined call — the timed region of
 * the reference's "Phasing time taken" span (floria.rs:330-337) with the pileups in host memory.  The cell arrays travel in
 * chunks of consecutive contigs and the blocks of a chunk start phasing when the chunk has landed, so most of the PCIe time
 * hides behind the kernels (needs sources in floria_hip_host_alloc memory; pageable sources are uploaded first, then phased).
 * keep == NULL: nothing stays resident.  keep != NULL: keep[0..n_contigs) receive the resident handles (floria_hip_contig_free
 * each), e.g. for floria_hip_hap_graph / S2 on the same batch.  Results are identical to upload + phase_blocks_batch. */
int  floria_hip_phase_pileups_batch(floria_hip_ctx* ctx, const floria_pileup* pileups, uint32_t n_contigs,
                                    const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end,
                                    uint32_t n_blocks, const floria_params* params, floria_block_result** out,
                                    floria_hip_contig** keep);

/* The compact wire form: bytes a packed copy of `in` needs (0 if `in` is malformed on its face: null field, first > last), and the
 * packing itself into caller memory (floria_hip_host_alloc memory for a DMA upload): *out receives views into buf.  Host-side, exact. */
size_t floria_hip_pack_bytes(const floria_pileup* in);
int    floria_hip_pack_pileup(const floria_pileup* in, void* buf, size_t buf_bytes, floria_pileup_packed* out);
/* The same for a batch of contigs, laid out field by field (all read_off arrays back to back, then all bit_off, ...): an upload of the batch
 * then is one transfer per field and chunk.  out[0..n) receive the views. */
size_t floria_hip_pack_bytes_batch(const floria_pileup* in, uint32_t n);
int    floria_hip_pack_pileups_batch(const floria_pileup* in, uint32_t n, void* buf, size_t buf_bytes, floria_pileup_packed* out);
/* floria_hip_contig_upload_batch / floria_hip_phase_pileups_batch from the compact form: same handles, same results, a fifth of the bytes
 * on the PCIe link. */
int  floria_hip_contig_upload_batch_packed(floria_hip_ctx* ctx, const floria_pileup_packed* pileups, uint32_t n, floria_hip_contig** out);
int  floria_hip_phase_pileups_batch_packed(floria_hip_ctx* ctx, const floria_pileup_packed* pileups, uint32_t n_contigs,
                                           const uint32_t* blk_contig, const uint32_t* blk_start, const uint32_t* blk_end,
                                           uint32_t n_blocks, const floria_params* params, floria_block_result** out,
                                           floria_hip_contig** keep);

/* S1 over MANY contigs in one launch sequence (the unit bench.py times: all blocks of all
 * contigs a rank owns are phased together so the device sees >> 256 concurrent jobs).
 * blk_contig[b] indexes `contigs`; results are in block order. */
int  floria_hip_phase_blocks_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs,
                                   uint32_t n_contigs, const uint32_t* blk_contig,
                                   const uint32_t* blk_start, const uint32_t* blk_end,
                                   uint32_t n_blocks, const floria_params* params,
                                   floria_block_result** out);

/* S2: process_reads_for_final_parts (part_block_manip.rs:174-274) with reassign_short = false
 * (the CLI default; the short-read branch :235-270 sits behind a hidden flag). */
int  floria_hip_reassign(floria_hip_ctx* ctx, const floria_hip_contig* contig,
                         const uint64_t* grp_off, const uint32_t* grp_read,
                         const uint32_t* grp_range, uint32_t n_groups, double epsilon,
                         floria_groups** out);
void floria_hip_groups_free(floria_groups* g);

/* S2 for many contigs in one launch (one wavefront per contig; the chain is sequential inside a contig and independent
 * across contigs).  grp_contig[g] indexes `contigs`; *out is an array of n_contigs floria_groups* in contig order. */
int  floria_hip_reassign_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                               const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                               const uint32_t* grp_range, uint32_t n_groups,
                               const uint32_t* read_order, const uint64_t* order_off,   /* both NULL, or see below */
                               double epsilon, floria_groups*** out);
/* The greedy re-insertion is strongly order-dependent and the reference visits reads in the iteration order of its
 * `read_to_parts_map: FxHashMap<&Frag, _>` (part_block_manip.rs:203).  A host that wants the reference's exact result passes
 * that order: read_order[order_off[c] .. order_off[c+1]) = counter_ids of contig c's reads in visiting order (every read that
 * sits in a group exactly once).  With NULL the reads are visited in ascending counter_id. */
int  floria_hip_reassign_ordered(floria_hip_ctx* ctx, const floria_hip_contig* contig,
                                 const uint64_t* grp_off, const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups,
                                 const uint32_t* read_order, uint32_t n_order, double epsilon, floria_groups** out);
void floria_hip_groups_array_free(floria_groups** arr, uint32_t n_contigs);

/* Nodes and edges of the hap graph for the batch `res` came from.  Must be called on the same context directly after the
 * floria_hip_phase_blocks* call that produced `res` (the block lists and partitions are still resident in HBM);
 * returns FLORIA_E_INVALID if the resident copy has been overwritten by a later call. */
int  floria_hip_hap_graph(floria_hip_ctx* ctx, const floria_block_result* res, floria_hap_graph** out);
void floria_hip_hap_graph_free(floria_hap_graph* g);

/* Coverage / error statistics of haplosets (utils_frags::get_errors_cov_from_frags, utils_frags.rs:596-655 — the COV and ERR
 * fields of the vartig / haploset headers): out4[4g..4g+3] = (cov, err, total_err, total_cov) of group g over its inclusive SNP
 * range.  err of an empty haploset is NaN, as in the reference (0/0). */
int  floria_hip_haploset_stats(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                               const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                               const uint32_t* grp_range, uint32_t n_groups, double* out4);

/* part_block_manip::get_hapq (part_block_manip.rs:517-616 — the HAPQ and REL_ERR fields of the vartig / haploset headers and the
 * avg_err column of the contig ploidy table) for the haplosets of one contig: groups are read-id lists (counter_ids) with their
 * inclusive 1-based SNP ranges; snp_to_genome_pos[s-1] is the base position of SNP s; block_length is the run's -l.
 * hapq[g] in 0..60, rel_err[g] = err_g / avg_err (NaN / inf exactly where the reference's f64 division gives them). */
int  floria_hip_hapq(floria_hip_ctx* ctx, const floria_hip_contig* contig,
                     const uint64_t* grp_off, const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups,
                     const uint64_t* snp_to_genome_pos, uint32_t n_snps, uint64_t block_length,
                     uint8_t* hapq, double* rel_err, double* avg_err);

/* The same for the haplosets of many contigs in one call (grp_contig[g] indexes `contigs`, pairs are searched inside a contig,
 * snp_to_genome_pos[c] / n_snps[c] / avg_err[c] are per contig): three launches for the whole run instead of three per contig. */
int  floria_hip_hapq_batch(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const uint32_t* grp_contig,
                           const uint64_t* grp_off, const uint32_t* grp_read, const uint32_t* grp_range, uint32_t n_groups,
                           const uint64_t* const* snp_to_genome_pos, const uint32_t* n_snps, uint64_t block_length,
                           uint8_t* hapq, double* rel_err, double* avg_err);

/* alignment::realign (alignment.rs:7-64) for many SNP calls at once: call i has the read's 32 bases around the SNP (read_windows[32 i ..],
 * A C G T, the SNP in column 16), the reference's 32 bases (ref_windows, upper case) and n_alleles[i] candidate bases (alleles[4 i ..], the
 * record's REF and ALTs in order).  best[i] = index of the FIRST allele whose window, with the allele in column 16, has the maximal global
 * alignment score against the read window (match +1, mismatch -1, gap open -2, extend -1).  score (may be NULL) receives that score.
 * The reference scores with block-aligner (an adaptive-band approximation); this is the exact affine-gap DP. */
int  floria_hip_realign(floria_hip_ctx* ctx, const uint8_t* read_windows, const uint8_t* ref_windows, const uint8_t* alleles,
                        const uint8_t* n_alleles, uint64_t n, uint8_t* best, int32_t* score);

/* The same calls scored by a FIXED-BLOCK WALK instead of the exact DP: a block of `block` x `block` cells starts at the top-left corner of the
 * alignment matrix and is shifted right or down by `step` cells until it holds the last cell; the direction compares the block's right border
 * column with its bottom border row (`rule` 0: their maxima, 1: their sums), ties go right (`tie` 0) or down (1); a cell whose neighbour was never
 * computed sees -infinity from it.  The definition is walk_score() of scripts/probes/block_walk.c; the result is bit-equal to it and never above
 * the exact score.  Supported members: block 8, step 1 | 2 | 4 | 8, rule 0 | 1, tie 0 | 1; anything else is FLORIA_E_INVALID.  The reference's
 * block-aligner (block size 8, alignment.rs:14) is SOME fixed-block heuristic; which member it is, if any, is unknown without the crate: the family
 * is selectable, nothing is pinned, and floria_hip_realign (the exact DP) stays the default everywhere. */
typedef struct floria_realign_walk { uint32_t block, step, rule, tie; } floria_realign_walk;
int  floria_hip_realign_walk(floria_hip_ctx* ctx, const uint8_t* read_windows, const uint8_t* ref_windows, const uint8_t* alleles,
                             const uint8_t* n_alleles, uint64_t n, const floria_realign_walk* walk, uint8_t* best, int32_t* score);

/* ---- frag_from_record (file_reader.rs:661-736) on the device: alignment records -> SNP calls ------------------------------------------------------
 * Alignment records as offsets into one byte blob. The blob may be an uncompressed BAM alignment section as it is
 * (offsets point into the records), or arrays the host packed itself. Nothing is assumed about alignment. */
typedef struct {
    const uint8_t*  blob;  uint64_t blob_bytes;
    uint32_t        n_records;
    const int32_t*  pos;        /* [n] 0-based leftmost reference position (BAM `pos`)                        */
    const uint16_t* flags;      /* [n] BAM FLAG; only 0x800 is read (leading hard clip of a supplementary)    */
    const uint32_t* contig;     /* [n] index into the SNP table                                               */
    const uint64_t* cigar_off;  /* [n] byte offset of n_cigar[i] little-endian u32 ops (len << 4 | op)        */
    const uint32_t* n_cigar;    /* [n]                                                                        */
    const uint64_t* seq_off;    /* [n] byte offset of (l_seq[i]+1)/2 bytes, two bases per byte, high nibble first (BAM) */
    const uint32_t* l_seq;      /* [n]                                                                        */
    const uint64_t* qual_off;   /* [n] byte offset of l_seq[i] quality bytes                                  */
} floria_alignments;

typedef struct {
    uint32_t        n_contigs;
    const uint64_t* snp_off;    /* [n_contigs+1]                                                              */
    const int64_t*  snp_pos;    /* 0-based genome positions, strictly ascending inside a contig; the SNP's    */
                                /* 1-based index (SnpPosition) is its rank in the contig + 1                  */
    const uint8_t*  alleles;    /* [4 * n_snps] the record's REF then ALT bases, as bytes                     */
    const uint8_t*  n_alleles;  /* [n_snps] 1..4                                                              */
} floria_snp_table;

typedef struct {               /* library-owned; record i owns cells [cell_off[i], cell_off[i+1]), ascending snp */
    uint32_t  n_records;
    uint64_t* cell_off;  uint32_t* snp;  uint8_t* allele;  uint8_t* qual;  uint32_t* seq_pos;
    int64_t*  ref_end;         /* [n] bam_endpos: pos + reference bases consumed (1 if none)                  */
} floria_record_cells;

/* One record's walk: a query cursor q = 0 and a reference cursor r = pos go through the CIGAR; for an M, = or X run [r, r + len) every SNP of the record's
 * contig with r <= snp_pos < r + len is visited: seq_pos = q + (snp_pos - r); if seq_pos < l_seq the base there is decoded with "=ACMGRSVTWYHKDBN", and if it
 * equals alleles[k] (as a byte) for some k < n_alleles, ONE cell is emitted for the first such k: snp = the SNP's rank in its contig + 1, allele = k, qual = the
 * quality byte at seq_pos, seq_pos = seq_pos plus the length of a leading H operation when flag 0x800 is set (modulo 2^32).  D and N advance r only (a SNP under
 * them yields nothing), I and S advance q only, H and P neither.  SNP indices are the table's own (snp_pos, alleles, n_alleles are indexed from 0, contig c
 * owning [snp_off[c], snp_off[c+1])).
 * The host part validates every input before anything is launched: every offset range against blob_bytes, contig < n_contigs, non-decreasing snp_off, strictly
 * ascending snp_pos inside a contig, n_alleles >= 1 (FLORIA_E_INVALID each) and n_alleles <= 4 (FLORIA_E_UNSUPPORTED, as elsewhere); the kernels
 * (csrc/pileup_kernel.h) bound every access by those lengths.  The blob and the arrays go up by DMA where they lie in floria_hip_host_alloc memory and through the
 * library's pinned staging ring otherwise; every result array comes back in one transfer.  floria_hip_last_timing then reports h2d_ms, d2h_ms, pileup_ms,
 * total_ms and upload_pinned_bytes / upload_staged_bytes of the call. */
int  floria_hip_pileup_records(floria_hip_ctx* ctx, const floria_alignments* alignments, const floria_snp_table* snps, floria_record_cells** out);
void floria_hip_record_cells_free(floria_record_cells* cells);

/* ---- the same walk with alignment::realign (alignment.rs:7-64) applied to its cells before they leave the device ----------------------------------------------
 * refs: one reference sequence per contig of the SNP table (contig c owns seq[seq_off[c] .. seq_off[c+1]); an empty one = the contig has no reference and none of
 * its cells is realigned).  Every field of the result equals floria_hip_pileup_records' except `allele`.  For a cell of record i with SNP index k, G = snp_pos[k],
 * p = the emitted seq_pos (hard-clip shift included, widened to 64 bits), L = l_seq[i] and R = the length of the contig's sequence:
 *   - the allele stays as walked unless 16 <= G, G + 16 < R, 16 <= p and p + 16 < L (compared in 64 bits);
 *   - q[j], j = 0..31, is the base of record i at index p - 16 + j (decoded with "=ACMGRSVTWYHKDBN"; anything but A, C, G, T becomes A), r[j] the upper-cased
 *     reference byte at G - 16 + j, al[m] = alleles[4k + m] upper-cased for m < n_alleles[k]; h = the number of columns j != 16 with q[j] != r[j];
 *   - h <= 2 and some al[m] == q[16]: the first such m; else h <= 1: 0; otherwise the first m with the maximal score of q against r with al[m] in column 16,
 *     scored as floria_hip_realign does (walk == NULL) or as floria_hip_realign_walk does for that member (anything else is FLORIA_E_INVALID).
 * counts (may be NULL): cells = all cells, in_bounds = those the bounds let through, shortcut / scored = how they were decided (in_bounds = shortcut + scored),
 * changed = cells whose allele differs from the walked one.
 * Validated on the host before any launch, beyond what floria_hip_pileup_records checks: refs->n_contigs == snps->n_contigs, non-decreasing seq_off, a non-null seq
 * when any contig is non-empty, the walk member.  The reference bytes go up with the other inputs; the gather, scoring and scatter kernels
 * (csrc/realign_gather_kernel.h) count into pileup_ms.  The call may reuse the buffer that holds the last phase_blocks* batch: like floria_hip_realign it ends that batch's
 * residency (floria_hip_hap_graph then returns FLORIA_E_INVALID for it); floria_hip_pileup_records does not. */
typedef struct { uint32_t n_contigs; const uint64_t* seq_off; /* [n_contigs+1] */ const uint8_t* seq; } floria_ref_seqs;
typedef struct { uint64_t cells, in_bounds, shortcut, scored, changed; } floria_realign_counts;
int  floria_hip_pileup_records_realign(floria_hip_ctx* ctx, const floria_alignments* alignments, const floria_snp_table* snps, const floria_ref_seqs* refs,
                                       const floria_realign_walk* walk /* NULL = exact DP */, floria_record_cells** out, floria_realign_counts* counts /* may be NULL */);

/* ---- records -> cells -> RESIDENT CONTIGS: the cells never leave the device ----------------------------------------------------------------------------------------
 * floria_hip_pileup_records_resident is floria_hip_pileup_records (refs == NULL: the walk alone) or floria_hip_pileup_records_realign (refs given; walk as there,
 * NULL = exact DP) with the same inputs, the same validation and the same kernels, but the per-cell arrays (snp, allele, qual, seq_pos) are NOT copied back: they
 * stay in the context's pileup buffers for floria_hip_assemble_contigs.  The library-owned summary holds what a host needs to plan fragments (header-sized, per
 * record): cell_off, the SNP of the record's first / last cell (0 / 0 for a record without cells), ref_end, and the realign counts (cells alone without refs).
 * Every value equals what floria_hip_pileup_records[_realign] returns for the same inputs.
 * RESIDENCY.  The context remembers `token`; the cells stay valid until the NEXT floria_hip_pileup_records, floria_hip_pileup_records_realign or
 * floria_hip_pileup_records_resident call on the context (each of them rewrites the pileup buffers, whether it succeeds or not) or floria_hip_destroy.  Nothing else
 * ends it: uploads, floria_hip_phase_*, floria_hip_reassign*, floria_hip_hap_graph, floria_hip_haploset_*, floria_hip_hapq*, floria_hip_realign* and
 * floria_hip_assemble_contigs itself work in other buffers, so one residency can be assembled any number of times.  Like floria_hip_pileup_records_realign the call
 * may end the residency of the last phase_blocks* batch (floria_hip_hap_graph) when refs are given.  The summary must stay alive (not freed) while it is used. */
typedef struct {
    uint32_t  n_records;
    uint64_t* cell_off;        /* [n+1] record i owns cells [cell_off[i], cell_off[i+1]) of the resident arrays       */
    uint32_t* first_snp;       /* [n]   1-based SNP index of the record's first cell, 0 if it has none                */
    uint32_t* last_snp;        /* [n]   ... of its last cell, 0 if it has none                                        */
    int64_t*  ref_end;         /* [n]   as floria_record_cells::ref_end                                               */
    floria_realign_counts counts;   /* as floria_hip_pileup_records_realign reports them; without refs only `cells`   */
    uint64_t  token;           /* identifies the device-resident cells (floria_hip_assemble_contigs)                  */
} floria_record_summary;
int  floria_hip_pileup_records_resident(floria_hip_ctx* ctx, const floria_alignments* alignments, const floria_snp_table* snps, const floria_ref_seqs* refs /* NULL = walk only */,
                                        const floria_realign_walk* walk /* NULL = exact DP */, floria_record_summary** out);
void floria_hip_record_summary_free(floria_record_summary* s);

/* ---- BGZF members inflated ON THE DEVICE: the record bytes never cross the link ---------------------------------------------------------------------------------------
 * floria_hip_inflate_bgzf inflates n_members BGZF members of a file image (file_bytes[0 .. n_bytes); member m is the member_bytes[m] bytes at member_off[m]) into a
 * floria_hip_blob: a device buffer of its own — creating, using or freeing it ends no residency — that holds the members' inflated bytes back to back in the order
 * given.  The compressed file is roughly a tenth of the inflated bytes a host would otherwise upload.
 * HOST PART, all of it before anything is uploaded or launched, FLORIA_E_INVALID naming the member: the offset range against n_bytes; the gzip header (magic, CM = 8,
 * FLG = FEXTRA, the BC subfield — other subfields may stand before it — and BSIZE against member_bytes); the CRC32 and ISIZE trailer is read, the output offsets are
 * the prefix sums of ISIZE.  ISIZE > 65 536 is FLORIA_E_UNSUPPORTED: a gzip file that is not BGZF.  The compressed bytes (from the first to the last member given) go
 * up by DMA where they lie in floria_hip_host_alloc memory and through the pinned staging ring otherwise.
 * KERNELS (csrc/inflate_kernel.h): raw DEFLATE (RFC 1951) per member — stored, fixed and dynamic blocks, any number of blocks — one wavefront per member in a
 * persistent grid, the member's output and the Huffman tables in LDS, one coalesced flush; then the CRC32 of every member's output.  Every input read is bounded by the
 * member's payload length, every output write by its ISIZE, every table index by its table, and every decoding step consumes an input bit or emits an output byte.
 * A per-member status word reports: bits ran out, reserved block type, LEN/NLEN mismatch, over-subscribed or incomplete code lengths, distance beyond the bytes
 * produced, output longer or shorter than ISIZE, CRC mismatch, invalid code.  Any non-zero status makes the call FLORIA_E_INVALID with the first such member and its
 * reason in the message; no handle is returned and the context stays usable.  The decoder is one host/device function template; tests/cpp/inflate_core_check.cpp runs
 * the same text on the CPU against zlib under the sanitizers.
 * floria_hip_last_timing then reports h2d_ms, pileup_ms (the two kernels), d2h_ms (the status words), total_ms and upload_pinned_bytes / upload_staged_bytes.
 * (Test option "inflate_slots" = N: at most N members in flight; 0 = default, two per CU.)
 * floria_hip_blob_download copies bytes [off, off + bytes) of the blob to the host: for tests, and for the rare host that needs a record's aux bytes. */
typedef struct floria_hip_blob floria_hip_blob;
int  floria_hip_inflate_bgzf(floria_hip_ctx* ctx, const uint8_t* file_bytes, uint64_t n_bytes, const uint64_t* member_off /* [n_members] */,
                             const uint32_t* member_bytes /* [n_members] */, uint32_t n_members, floria_hip_blob** out);
uint64_t floria_hip_blob_bytes(const floria_hip_blob* blob);
int  floria_hip_blob_download(const floria_hip_blob* blob, uint64_t off, void* dst, uint64_t bytes);
void floria_hip_blob_free(floria_hip_blob* blob);

/* The header-sized record table of a blob that holds BAM alignment records.  Chain c starts at byte begin[c] and follows the block_size prefixes while a whole record
 * fits before end[c], one lane per chain (a host with a .bai gives one chain per contig; without an index there is one chain per segment); a second pass, one thread
 * per record (count, scan, fill), returns per record the offset of its block_size prefix, block_size, refID, pos, mapq, flag, n_cigar_op, l_seq, l_read_name and its
 * first CIGAR word (0 for a record without CIGAR), by which a host recognises the kSmN placeholder of a CG-tag record, and the names, compacted into one byte array
 * (record i owns names[name_off[i] .. name_off[i + 1]): the l_read_name bytes as stored, the closing NUL included).  Records stand chain by chain: chain c owns records
 * chain_rec_off[c] .. chain_rec_off[c + 1]; chain_stop[c] is the offset where it stopped.  From offset, l_read_name, n_cigar_op and l_seq the host computes
 * cigar_off = offset + 36 + l_read_name, seq_off = cigar_off + 4 n_cigar_op and qual_off = seq_off + (l_seq + 1) / 2 itself.
 * A block_size below the 32 fixed bytes of a record, or one that runs past end[c] (or a prefix cut by it), stops the chain: FLORIA_E_INVALID naming chain and offset —
 * a chain that stops exactly at end[c] is complete.  Refused before any launch, FLORIA_E_INVALID: a null argument, a blob of another context, begin[c] > end[c] or
 * end[c] past the blob.  FLORIA_E_UNSUPPORTED: 2^32 and more records.  The call works in buffers of its own and ends no residency; floria_hip_last_timing then reports
 * pileup_ms (the kernels), h2d_ms, d2h_ms, total_ms.
 * OPEN-ENDED CHAINS (floria_hip_blob_records_opt; flags == 0 is floria_hip_blob_records, which calls it): a tool does not know where a chain ends — a .bai gives the
 * end of a target as a hint, and a streamed file is cut at member boundaries, inside a record and inside a target.  Two flags, independent of each other:
 *   FLORIA_CHAIN_CUT_TAIL  a block_size prefix or a record cut by end[c] ends the chain without an error; chain_stop[c] is the offset of that prefix, the first byte
 *                          not consumed.  A block_size below 32 stays FLORIA_E_INVALID naming chain and offset.
 *   FLORIA_CHAIN_ONE_REF   the chain ends in front of the first record whose refID differs from that of its first record (chain_stop[c] is that record's offset).
 *                          The refID is read only after the fit checks have shown the record to lie before end[c]; with both flags a record cut by end[c] therefore
 *                          ends the chain as a cut tail whatever its refID.
 * chain_why[c] says how chain c ended: 0 it reached end[c] exactly, 1 cut tail, 2 another reference.  Any other flag bit is FLORIA_E_INVALID. */
#define FLORIA_CHAIN_CUT_TAIL 1u
#define FLORIA_CHAIN_ONE_REF  2u
typedef struct {
    uint32_t  n_chains;
    uint64_t  n_records;
    uint64_t* chain_rec_off;   /* [n_chains+1] */
    uint64_t* chain_stop;      /* [n_chains]   */
    uint64_t* offset;          /* [n] byte offset of the record's block_size prefix in the blob */
    uint32_t* block_size;      /* [n] */
    int32_t*  ref_id;          /* [n] */
    int32_t*  pos;             /* [n] */
    uint32_t* l_seq;           /* [n] */
    uint32_t* cigar0;          /* [n] the first CIGAR word (len << 4 | op), 0 if n_cigar_op == 0 */
    uint16_t* flag;            /* [n] */
    uint16_t* n_cigar_op;      /* [n] */
    uint8_t*  mapq;            /* [n] */
    uint8_t*  l_read_name;     /* [n] */
    uint64_t* name_off;        /* [n+1] */
    uint8_t*  names;           /* [name_off[n]] */
    uint32_t* chain_why;       /* [n_chains] 0 = reached end[c], 1 = cut tail, 2 = another reference (appended: the struct is library-allocated) */
} floria_blob_records;
int  floria_hip_blob_records(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* begin /* [n_chains] */, const uint64_t* end /* [n_chains] */,
                             uint32_t n_chains, floria_blob_records** out);
int  floria_hip_blob_records_opt(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* begin /* [n_chains] */, const uint64_t* end /* [n_chains] */,
                                 uint32_t n_chains, uint32_t flags /* FLORIA_CHAIN_* */, floria_blob_records** out);
void floria_hip_blob_records_free(floria_blob_records* r);

/* The bases and qualities of n records of a blob in one call, as the read writers want them: record i has its packed bases, (l_seq[i] + 1) / 2 bytes, at seq_off[i] and
 * its l_seq[i] quality bytes at qual_off[i] (the offsets floria_hip_blob_records' header comment derives; any alignment, l_seq may be 0 or odd).  Record i owns bytes
 * [base_off[i], base_off[i + 1]) of `bases` and of `quals`; base_off is the prefix sum of l_seq.  A base is the 4-bit code 1 / 2 / 4 / 8 as 'A' / 'C' / 'G' / 'T' and
 * 'A' for every other code; the padding nibble of an odd l_seq does not appear.  A quality is q > 222 ? 255 : q + 33.  (csrc/blob_seq_kernel.h: one wavefront per
 * record, the output written in 8-byte words between a byte-wise head and tail.)
 * Refused before any launch, FLORIA_E_INVALID: a null argument, a blob of another context, a sequence or quality range that reaches past the blob (the message names
 * the record).  FLORIA_E_UNSUPPORTED: 2^32 and more records, or bases in total.  The call works in buffers of its own and ends no residency; floria_hip_last_timing then
 * reports pileup_ms (the kernel), h2d_ms, d2h_ms, total_ms. */
typedef struct {
    uint64_t  n;
    uint64_t* base_off;        /* [n+1] */
    uint8_t*  bases;           /* [base_off[n]] */
    uint8_t*  quals;           /* [base_off[n]] */
} floria_blob_sequences;
int  floria_hip_blob_sequences(floria_hip_ctx* ctx, const floria_hip_blob* blob, const uint64_t* seq_off /* [n] */, const uint32_t* l_seq /* [n] */,
                               const uint64_t* qual_off /* [n] */, uint64_t n, floria_blob_sequences** out);
void floria_hip_blob_sequences_free(floria_blob_sequences* r);

/* The -e / -l estimate (file_reader.rs:749-826) on records of a blob (csrc/estimate_kernel.h).  The caller has filtered the records (refID >= 0, (flag & 1796) == 0,
 * at least one CIGAR operation) and gives them in groups, one group per contig in header order, ascending by pos inside a group; record i has its n_cigar[i] CIGAR
 * words at cigar_off[i] (a CG:B,I array's for a record with the kSmN placeholder) and its packed bases, (l_seq[i] + 1) / 2 bytes, at seq_off[i].
 * THE FUNCTION: record i spans [pos, end), end = pos + (sum of the lengths of its M D N = X operations), pos + 1 where that sum is 0.  Every position of a group that
 * lies in a span is a column; the columns of all groups, ascending inside a group, are one sequence.  `count` and `n_err` run through it: a column met with
 * count % 1000 != 0 only advances count; otherwise it is SAMPLED: every record whose span holds it and whose operation there is M, = or X gives the 4-bit code at its
 * query offset, if that offset is below l_seq; total = the bases given, most = the largest number of equal codes.  total < 5: count stays (the next column is sampled
 * too); else n_err advances, the call is `done` where n_err reaches `stop`, and count advances otherwise.
 * WHAT COMES BACK: every sampled column in order — its group, position, total and most, those with total < 5 too — and rec_hits[i], the number of sampled columns
 * (up to the one that reached stop) record i gave a base to; the state after the last column in *inout, so that a second call over the records that follow
 * continues the sequence.  The host forms (total - most) / most of the columns with total >= 5, the multiset of l_seq by rec_hits, and the percentiles.
 * inout->n_err >= stop on entry: an empty result with done = 1, nothing launched.
 * Memory is linear in a position window: a group is walked in windows of at most 2^22 positions (test option "estimate_window" = N, 1 .. 2^30), every window
 * over the records whose span meets it, the state carried from one to the next; the split changes no result.
 * Refused before any launch, FLORIA_E_INVALID, the message naming the record or group: a null argument, a blob of another context, group_off not starting at 0, descending
 * or not ending at n, n_cigar == 0, a negative pos, pos descending inside a group, a CIGAR or sequence range that reaches past the blob.  FLORIA_E_UNSUPPORTED: 2^32 and
 * more records; after the span pass, an end beyond 2^31 - 1.  The call works in buffers of its own and ends no residency; floria_hip_last_timing then reports pileup_ms
 * (all kernels), h2d_ms, d2h_ms, total_ms. */
typedef struct {
    uint64_t n;
    const int32_t*  pos;        /* [n] */
    const uint64_t* cigar_off;  /* [n] */
    const uint32_t* n_cigar;    /* [n] */
    const uint64_t* seq_off;    /* [n] */
    const uint32_t* l_seq;      /* [n] */
    uint32_t n_groups;
    const uint64_t* group_off;  /* [n_groups+1] */
} floria_estimate_records;
typedef struct { uint64_t count; uint32_t n_err; } floria_estimate_state;
typedef struct {               /* library-owned */
    uint64_t  n_cols;
    uint32_t* col_group;       /* [n_cols] every sampled column in order, the discarded ones (total < 5) too */
    int32_t*  col_pos;
    uint32_t* col_total;
    uint32_t* col_most;
    uint32_t* rec_hits;        /* [n] sampled columns record i gave a base to */
    uint32_t  done;            /* n_err reached stop */
} floria_estimate_result;
int  floria_hip_blob_estimate(floria_hip_ctx* ctx, const floria_hip_blob* blob, const floria_estimate_records* records, uint32_t stop, floria_estimate_state* inout,
                              floria_estimate_result** out);
void floria_hip_estimate_result_free(floria_estimate_result* r);

/* floria_hip_pileup_records_resident whose record bytes are a blob handle: alignments->blob must be NULL (FLORIA_E_INVALID otherwise), alignments->blob_bytes is
 * ignored and the offsets index the handle.  The same validation, against the handle's length; the same kernels, pointed at the handle's buffer; the same summary,
 * token and RESIDENCY rule; no record byte is uploaded.  A blob of another context is FLORIA_E_INVALID.  The blob must stay alive while the call runs; the residency
 * does not need it afterwards (the cells are in the context's pileup buffers). */
int  floria_hip_pileup_records_resident_blob(floria_hip_ctx* ctx, const floria_hip_blob* blob, const floria_alignments* alignments, const floria_snp_table* snps,
                                             const floria_ref_seqs* refs /* NULL = walk only */, const floria_realign_walk* walk /* NULL = exact DP */, floria_record_summary** out);

/* A fragment plan: which records of the resident call form a fragment (a `Frag` after combine_frags, file_reader.rs:539-541 and :636-639), in which order they
 * are merged, and in which order the fragments of a contig stand.  All of it follows from names, flags and the per-record spans of the summary. */
typedef struct {
    uint32_t        n_contigs;   /* == the SNP table's n_contigs of the resident pileup call; plan contig c is table contig c */
    const uint64_t* frag_off;    /* [n_contigs+1]  fragments of contig c, in the pileup's read order (Frag::cmp) */
    const uint64_t* part_off;    /* [n_frags+1]    into part_rec */
    const uint32_t* part_rec;    /* record indices of the resident call, in MERGE order: the first is the base, each later one is `extend`ed onto it */
    const uint32_t* set_order;   /* optional, NULL = not given: as floria_pileup::set_order, indexed by the MERGED cells of all contigs back to back */
} floria_fragment_plan;

/* combine_frags on the device: out[c] (c < plan->n_contigs) receives a resident contig whose read r is fragment frag_off[c] + r of the plan.
 *   - a fragment's cells: one cell per SNP that occurs in any of its parts, in ascending SNP order; allele and qual of a SNP come from the LAST part in list order
 *     that has it (`seq_dict.extend`: the later record's call overwrites the earlier one);
 *   - first / last: the smallest / largest merged SNP (= the min of the parts' firsts / max of their lasts; a part without cells changes neither);
 *   - seq_pos and ref_end are not part of a contig (floria_hip_assemble_contigs_opt keeps seq_pos); records the plan does not name are unused; a record may appear anywhere, any number of times; parts need not
 *     be in genome order.
 * The handles are indistinguishable from those floria_hip_contig_upload_batch returns for the equivalent floria_pileup array: every floria_hip_contig_download
 * field has the same bytes, the derived properties (biallelic / q = 0 routing, set_order in "arith" = 1, one arena for the batch) are the same, each is freed with
 * floria_hip_contig_free and every entry point that takes a contig takes them.  The merged cells are written into an arena laid out as an upload's
 * (csrc/assemble_kernel.h) and then validated and flattened by the upload's own kernel, so everything a host upload validates is validated here with the same
 * messages: Frag::cmp order of the fragments, ascending cells, 1-based SNPs, allele <= 3.  A contig without fragments is a pileup with n_reads == 0.
 * Checked on the host before anything is launched, FLORIA_E_INVALID each: a null argument; `resident` is not the context's live residency (see above); n_contigs
 * differs from the resident call's; frag_off / part_off not starting at 0 or not ascending; a fragment with no part; a part_rec index >= n_records; a part whose
 * record belongs to another contig than its fragment; a fragment whose parts have no cell at all ("every read has >= 1 cell").  FLORIA_E_UNSUPPORTED: 2^32 and more
 * cells in one contig (as upload), 2^32 and more fragments.  With a set_order the cell orders are computed at once (the kernels "arith" = 1 runs before S1) and one
 * that is not a permutation of a fragment's cell indices is FLORIA_E_INVALID with the message S1 gives for an uploaded one.  On error no handle is returned and the
 * residency stays.  floria_hip_last_timing then reports pileup_ms (merge passes + scan), select_ms (flatten), h2d_ms, d2h_ms, total_ms. */
int  floria_hip_assemble_contigs(floria_hip_ctx* ctx, const floria_record_summary* resident, const floria_fragment_plan* plan, floria_hip_contig** out /* [n_contigs] */);

/* floria_hip_assemble_contigs whose set orders come from the device: the same validation, kernels, arena and handles, and in addition every contig that is MERGED —
 * that holds at least one fragment with two or more parts that have cells, which a host can tell from the summary's cell_off — carries a set_order
 * (floria_pileup::set_order) computed for every one of its reads as the reference's containers build Frag.positions (csrc/assemble_order_kernel.h):
 *   - each part's own set: an empty map receives the part's SNPs ascending, growing as it goes; an empty set reserves room for all of them and receives the map's
 *     keys in bucket order; a part without cells leaves the unallocated empty set;
 *   - the accumulator starts as the first part's set; for every later part reserve(accumulator empty ? n : (n + 1) / 2), then insert of the part's keys in the
 *     iteration order of the part's own set — insert reserves room for one key before it looks the key up, so a key both parts have can still grow a full table;
 *   - set_order[read_off[r] + j] = the index within the merged read of the j-th key in the accumulator's bucket order.
 * Contigs that are not merged carry no set_order and every download field of theirs has the bytes the plain call gives; if no contig is merged the call IS the
 * plain call.  The derived orders lie where an uploaded set_order lies, the cell orders are computed at once as for a host-given order (their permutation check
 * covers the derived orders too), and "arith" = 1 and floria_hip_drop_monomorphic(.., with_set_order = 1) use them as they use a host-given one.
 * plan->set_order != NULL is FLORIA_E_INVALID before anything is launched (give the order or ask for it, not both).  Fragments whose parts have more than 223
 * cells together take a one-thread-per-fragment kernel whose tables are sized from the summary before any launch: FLORIA_E_NOMEM if they cannot be had,
 * FLORIA_E_UNSUPPORTED for 2^31 and more cells in the parts of one fragment.  On error no handle is returned and the residency stays.  floria_hip_last_timing
 * counts the additional launches into pileup_ms.  (Test option "asm_order_general" = 1: every fragment takes the one-thread kernel; results do not change.) */
int  floria_hip_assemble_contigs_ordered(floria_hip_ctx* ctx, const floria_record_summary* resident, const floria_fragment_plan* plan, floria_hip_contig** out /* [n_contigs] */);

/* floria_hip_assemble_contigs with options.  flags == 0 IS floria_hip_assemble_contigs, flags == FLORIA_ASM_DERIVE_SET_ORDER IS floria_hip_assemble_contigs_ordered: the
 * same bytes in every handle, the same refusals with the same messages.
 * FLORIA_ASM_KEEP_SEQ_POS: every contig of the batch (an empty one too) CARRIES POSITIONS — Frag::snp_pos_to_seq_pos, one SEQ_POS word per resident cell:
 *     word = mate << 31 | seq_pos
 *   - seq_pos is what floria_record_cells::seq_pos holds for the cell that gave the merged SNP its call (hard-clip shift of a supplementary alignment included);
 *   - mate is part_mate[p] of the part p that cell belongs to — the second element of the reference's (u8, GnPosition): 1 for the parts the host marks as the
 *     second mate (file_reader.rs:556-562), 0 otherwise and for supplementary parts (:649-651); part_mate == NULL: every mate is 0;
 *   - a SNP several parts have takes the word of the LAST part in list order that has it (`snp_pos_to_seq_pos.extend` follows the rule of `seq_dict.extend`).
 * The words lie in a region of their own behind every other region of the arena; every other download field, the derived properties and the results of every
 * entry point on such a handle are those of the handle without positions.  floria_hip_contig_download(FLORIA_FIELD_SEQ_POS) returns the words,
 * floria_hip_drop_monomorphic carries them through, floria_hip_read_spans answers write_reads' two lookups from them.  Both flags together work: the set-order
 * kernels do not read positions.  A walked seq_pos >= 2^31 cannot be encoded (no BAM record with l_seq < 2^31 - 2^28 produces one): the FILL pass raises a status
 * word and the call fails with FLORIA_E_UNSUPPORTED, returns no handle and leaves the residency intact.
 * Refused before any launch, FLORIA_E_INVALID each: opts == NULL; flag bits other than the two; part_mate without FLORIA_ASM_KEEP_SEQ_POS; a part_mate byte other
 * than 0 or 1; everything the plain and the ordered call refuse. */
#define FLORIA_ASM_DERIVE_SET_ORDER 1u   /* what floria_hip_assemble_contigs_ordered does */
#define FLORIA_ASM_KEEP_SEQ_POS     2u
typedef struct { uint32_t flags; const uint8_t* part_mate; /* [n_parts] 0/1 in the order of part_rec, NULL = all 0; only with KEEP_SEQ_POS */ } floria_assemble_options;
int  floria_hip_assemble_contigs_opt(floria_hip_ctx* ctx, const floria_record_summary* resident, const floria_fragment_plan* plan, const floria_assemble_options* opts,
                                     floria_hip_contig** out /* [n_contigs] */);

/* ---- remove_monomorphic_allele (utils_frags.rs:713-772, --ignore-monomorphic; called at floria.rs:315-317) on resident contigs: no cell crosses the link ------------
 * contigs[0..n_contigs) are resident contigs of this context from any source (single uploads, an upload batch, floria_hip_assemble_contigs; they need not share an
 * arena); snp_off is the prefix sum of their SNP counts (contig c has SNPs 1 .. snp_off[c+1] - snp_off[c]).  Literal to the reference:
 *   counts    per SNP and allele 0..3 the sum of the cells' weights — the Q24 field of CELL_AW, i.e. phred_scale (utils_frags.rs:702-711) as an exact integer, so
 *             the sum is exact and order-free — and whether any cell calls the allele at all: a q = 0 cell weighs 0 but still makes its allele a key of the
 *             reference's map;
 *   decision  no allele present: the SNP stays (it is not in the map); exactly one: removed; otherwise, with v0 >= v1 the two largest sums as f64
 *             ((double)S * 2^-24, exact below 2^53), removed iff v0 * error > v1, strictly, in f64: equality keeps the SNP;
 *   reads     a read keeps its cells at surviving SNPs, in order, CELL_AW unchanged; first / last become its first / last surviving SNP; a read left without cells
 *             is dropped; the survivors are ordered by (new first ascending, new last descending, old read index ascending) — Frag::cmp with the old counter_id —
 *             and renumbered.
 * out[0..n_contigs) receive the output contigs: ONE new batch arena laid out as an upload's, every floria_hip_contig_download field (TW and META recomputed from
 * the surviving cells) byte for byte what floria_hip_contig_upload_batch produces for the equivalent filtered pileups, the derived properties (cells, longest read,
 * biallelic / q = 0 routing: "some surviving weight is 0") the same; each is freed with floria_hip_contig_free.  A contig that loses every read, or had none, yields
 * a handle with n_reads == 0.  The inputs are not touched and stay the caller's.
 * with_set_order != 0: every output contig carries a set_order (floria_pileup::set_order): per read the input read's iteration order — the host-given one where the
 * input contig has a set_order, else the one the library emulates for a one-walk set (csrc/arith_kernel.h) — with the removed cells deleted and the remaining
 * indices renumbered, which is what the reference's set holds (`remove` moves no other key, utils_frags.rs:745-755).  A host-given input order that is no
 * permutation is FLORIA_E_INVALID with S1's message.  with_set_order == 0: the outputs carry none, and "arith" = 1 on them then emulates a one-walk set of the
 * CUT-DOWN cells, which is NOT the reference's function for a read that lost cells (its set keeps the layout it had with the removed keys in it).
 * POSITIONS.  An output contig carries positions (floria_hip_assemble_contigs_opt) iff its input contig does: the surviving cells' SEQ_POS words move with them (the
 * reference removes the key from snp_pos_to_seq_pos with the cell, utils_frags.rs:749); the outputs of inputs without positions refuse FLORIA_FIELD_SEQ_POS as before.
 * res (may be NULL) receives the library-owned map back to the inputs (floria_hip_mono_result_free).
 * Refused before any launch, FLORIA_E_INVALID each: a null argument; a contig of another context; snp_off not starting at 0 or descending; a non-finite error; a
 * contig with a read whose `last` exceeds its SNP count (the message names the contig).  On error no handle is returned.
 * floria_hip_last_timing then reports pileup_ms (all device work of the call: see floria_hip_mono_timing), h2d_ms, d2h_ms, total_ms. */
typedef struct {
    uint32_t  n_contigs;
    uint64_t* read_off;     /* [n_contigs+1] reads of output contig c are old_read[read_off[c] .. read_off[c+1])            */
    uint32_t* old_read;     /* [read_off[n]] output read r of contig c was input read old_read[read_off[c]+r] of contig c   */
    uint8_t*  removed;      /* [snp_off[n]]  removed[snp_off[c] + s-1] = 1 iff SNP s (1-based) of contig c was removed      */
    uint64_t  n_removed_snps, n_removed_cells, n_dropped_reads;
    uint32_t* new_first;    /* [read_off[n]] first SNP of output read r of contig c after the removal, at read_off[c]+r: what FLORIA_FIELD_FIRST of out[c] holds   */
    uint32_t* new_last;     /* [read_off[n]] ... its last SNP (FLORIA_FIELD_LAST): a host that keeps headers only re-maps them without a download                    */
} floria_mono_result;
int  floria_hip_drop_monomorphic(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                 const uint64_t* snp_off /* [n_contigs+1], prefix sums of the contigs' SNP counts */,
                                 double error, int with_set_order,
                                 floria_hip_contig** out /* [n_contigs] */, floria_mono_result** res /* may be NULL */);
void floria_hip_mono_result_free(floria_mono_result* r);
/* pileup_ms of the context's last floria_hip_drop_monomorphic call by kind, in ms (hipEvents): ms6[0] clearing the tables, [1] the count pass, [2] the decision,
 * [3] filter COUNT, [4] filter FILL, [5] the set orders (the input orders through S1's kernels + their filtering; 0 without with_set_order). */
int  floria_hip_mono_timing(const floria_hip_ctx* ctx, double* ms6);

/* Allele tables of haplosets for a host that holds no cells (the allele strings of .vartigs / vartig_info.txt): the groups are given as for
 * floria_hip_haploset_stats; counts[4 * (pos_off[g] + (p - lo_g)) + a] = the number of group g's reads that call allele a at SNP p of its inclusive range
 * [lo_g, hi_g] — set_to_seq_dict(.., false) restricted to the range, what write_fragset_haplotypes (file_writer.rs:308-369) iterates.  pos_off [n_groups+1] is the
 * caller's prefix sum of the range lengths (hi - lo + 1, 0 for a group with hi < lo; anything else is FLORIA_E_INVALID); counts has 4 * pos_off[n_groups] entries.
 * Cells outside the range are ignored; a group with hi < lo or without reads contributes nothing.  Consensus and formatting stay on the host.  Like
 * floria_hip_haploset_stats the call works in the buffer that holds the last phase_blocks* batch and ends that batch's residency (floria_hip_hap_graph). */
int  floria_hip_haploset_alleles(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                 const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                                 const uint32_t* grp_range, uint32_t n_groups, const uint64_t* pos_off, uint32_t* counts);

/* The two lookups write_reads (file_writer.rs:460-530) makes in Frag::snp_pos_to_seq_pos per (haploset, read), for a host that holds no cells: the groups are given
 * as for floria_hip_haploset_alleles (reads of a contig plus an inclusive 1-based SNP range [lo, hi]); every contig must carry positions
 * (floria_hip_assemble_contigs_opt with FLORIA_ASM_KEEP_SEQ_POS, or floria_hip_drop_monomorphic of such contigs).  For entry j of group g (read grp_read[j] of contig
 * grp_contig[g]): left[j] = the SEQ_POS word (mate << 31 | seq_pos) of the read's first cell with snp >= lo, right[j] = that of its last cell with snp <= hi, each
 * FLORIA_SPAN_NONE where the read has no such cell.  The two are answered independently: a group with hi < lo gets no special case.  (The word of mate 1 at
 * seq_pos 2^31 - 1 equals FLORIA_SPAN_NONE; no BAM record reaches it.)  The +-25-base extension, extend_read_clipping and the sequence-length clamps stay on the host.
 * 8 B per entry come back, one transfer per array (csrc/span_kernel.h: one thread per entry, no scratch).
 * Refused before any launch, FLORIA_E_INVALID each: a null argument; a contig of another context; a contig without positions ("the contig carries no seq_pos");
 * grp_contig >= n_contigs; grp_off not starting at 0 or descending; a grp_read >= its contig's n_reads.
 * The call works in a buffer of its own: unlike floria_hip_haploset_alleles it ends no residency (the last phase_blocks* batch stays valid for floria_hip_hap_graph,
 * a record residency for floria_hip_assemble_contigs*).  floria_hip_last_timing then reports pileup_ms (the kernel), h2d_ms, d2h_ms, total_ms. */
#define FLORIA_SPAN_NONE 0xFFFFFFFFu
int  floria_hip_read_spans(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                           const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                           const uint32_t* grp_range, uint32_t n_groups, uint32_t* left /* [grp_off[n_groups]] */, uint32_t* right /* same */);

/* ---- S2 whose result stays on the device: haplosets as a handle ------------------------------------------------------------------------------------------------------
 * floria_hip_reassign_batch_resident is floria_hip_reassign_batch — the same arguments, the same validation and refusals with the same messages, the same host
 * prologue, the same re-insertion kernels with the same path choice in both arithmetics — but what follows the kernel (the groups from the per-read assignment,
 * separate_broken_haplogroups, sort_parts) runs on the device (csrc/haploset_kernel.h) and the result is a floria_hip_haplosets handle: for the n_contigs contigs
 * of the call, back to back in contig order, the group tables the consumer kernels read (grp_contig, grp_off, grp_read, range).  Group order and contents are those
 * floria_hip_reassign_batch returns, under "s2_assign_only" = 1 too; nothing depends on the order in which anything lands on the device.  One copy comes back during
 * the call: two words per contig (its groups, its reads).
 * RESIDENCY.  The handle lives in a buffer of its own and remembers the context and the contig handles it was made from (they must outlive it).  Creating, using
 * or freeing it ends no other residency beyond what the call it replaces ends (the S2 call itself works in the buffer of the last phase_blocks* batch, as
 * floria_hip_reassign_batch does), and no later call overwrites it: it answers the same after any number of S1 / S2 calls.
 * floria_hip_haplosets_download returns exactly what floria_hip_reassign_batch returns for the same inputs (floria_hip_groups_array_free); nothing goes back up.
 * The consumers by handle take (ctx, contigs, n_contigs, hs, ...) and otherwise the arguments of their siblings, run the siblings' kernels on the handle's arrays
 * — no group list is uploaded, no host loop touches a read — and return, bit for bit, what the sibling returns for the downloaded groups concatenated in contig
 * order (grp_contig[g] = the contig, grp_off rebased).  Their host parts read a header-sized mirror of the handle (grp_off and range, 16 B per group, fetched once
 * per handle; floria_hip_hapq_batch_resident also the SNP span of every group's reads, 8 B per group, computed by one launch).  pos_off of the alleles call is the
 * caller's, from the ranges of the download.
 * Buffers: floria_hip_haploset_stats_resident, floria_hip_haploset_alleles_resident and floria_hip_hapq_batch_resident work in the buffer their siblings use and
 * end the residency of the last phase_blocks* batch (floria_hip_hap_graph) as they do; floria_hip_read_spans_resident, floria_hip_haplosets_download and
 * floria_hip_haplosets_free end none.
 * Refused before any launch, FLORIA_E_INVALID each: a null argument; a handle of another context; a `contigs` array that is not the handle's (its count or any
 * pointer); for the spans call a contig without positions ("the contig carries no seq_pos").  floria_hip_last_timing after the S2 call: reassign_ms = the
 * re-insertion kernels, select_ms = the epilogue's kernels, h2d_ms, d2h_ms, total_ms. */
typedef struct floria_hip_haplosets floria_hip_haplosets;
int  floria_hip_reassign_batch_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                        const uint32_t* grp_contig, const uint64_t* grp_off, const uint32_t* grp_read,
                                        const uint32_t* grp_range, uint32_t n_groups,
                                        const uint32_t* read_order, const uint64_t* order_off,
                                        double epsilon, floria_hip_haplosets** out);
void floria_hip_haplosets_free(floria_hip_haplosets* hs);
int  floria_hip_haplosets_download(const floria_hip_haplosets* hs, floria_groups*** out /* [n_contigs of the S2 call] */);
int  floria_hip_haploset_stats_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs, double* out4);
int  floria_hip_hapq_batch_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs,
                                    const uint64_t* const* snp_to_genome_pos, const uint32_t* n_snps, uint64_t block_length,
                                    uint8_t* hapq, double* rel_err, double* avg_err);
int  floria_hip_haploset_alleles_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs,
                                          const uint64_t* pos_off, uint32_t* counts);
int  floria_hip_read_spans_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs, const floria_hip_haplosets* hs,
                                    uint32_t* left, uint32_t* right);

/* ---- hap-graph paths -> haplosets on the device, and S2 whose input is a handle: no per-read list crosses the link between S1 and S2 ------------------------------
 * floria_hip_join_paths is the union that ends get_disjoint_paths_rewrite (graph_processing.rs), on the S1 batch `res` that is still resident: path p (of contig
 * path_contig[p], non-descending) is the list of hap-graph nodes node_off[p] .. node_off[p + 1], node n = partition node_part[n] of block node_block[n] of that batch.
 * Group p of the result holds, ascending and once each, every read r for which some node (b, k) of the path has r in block b's list with part == k; its range is
 * path_range[2p], path_range[2p + 1], passed through.  A node may occur in several paths and a read in several groups; a path without nodes is an empty group that
 * keeps its range.  The result is a complete floria_hip_haplosets — the layout of the S2 handle, a buffer of its own, groups contig-major in path order — that
 * floria_hip_haplosets_download, the four *_resident consumers and floria_hip_reassign_haplosets_resident take as they take S2's.
 * RESIDENCY.  The token rule and message of floria_hip_hap_graph; the call may run before or after it, any number of times, and ends no residency (its tables lie in
 * buffers of their own).  `contigs` must be the array of the S1 call.
 * Kernels (csrc/path_kernel.h): per path an id window from its nodes' lists, a bitmap over it marked by integer atomicOr, popcount, prefix sums, fill by prefix
 * popcount: the result does not depend on the order in which anything lands; memory is linear in the sum of the windows.  Two copies come back during the call: the
 * bitmap's size (8 B) and two words per contig.
 * Refused before any launch, FLORIA_E_INVALID each, the message naming the argument: a null argument; a stale or foreign token; a contig of another context or an
 * array that is not the S1 call's; path_contig >= n_contigs or descending; node_off not starting at 0 or descending; node_block >= n_blocks; node_part >=
 * best_ploidy[block] (which covers every node of an empty block); a node whose block belongs to another contig than its path.
 *
 * floria_hip_reassign_haplosets_resident is floria_hip_reassign_batch_resident whose input groups are the handle `in` (from floria_hip_join_paths or from an S2 call;
 * it is left unchanged and valid): floria_hip_haplosets_download(*out) equals, list for list, what floria_hip_reassign_batch_resident returns for
 * floria_hip_haplosets_download(in) concatenated in contig order with read_order == NULL — in both arithmetics, under "s2_assign_only" and under "reassign_path" 1
 * and 2.  Reads are visited in ascending counter_id.  The per-read tables of the prologue (read -> candidate groups, the `multi` list, the id windows) are built on
 * the device from the handle (csrc/haploset_kernel.h); the host reads header-sized data only: per group its size and the SNP span of its reads, per contig the number
 * of reads that have a choice.  Re-insertion kernels, path choice and epilogue are those of floria_hip_reassign_batch_resident.  Like it, the call works in the buffer
 * of the last phase_blocks* batch and ends that batch's residency.  Refused as the *_resident consumers refuse: a null argument, a handle of another context, a
 * `contigs` array that is not the handle's. */
int  floria_hip_join_paths(floria_hip_ctx* ctx, const floria_block_result* res,
                           const floria_hip_contig* const* contigs, uint32_t n_contigs,
                           const uint32_t* path_contig,   /* [n_paths] index into contigs, non-descending */
                           const uint64_t* node_off,      /* [n_paths+1] */
                           const uint32_t* node_block,    /* [node_off[n_paths]] block index of the S1 batch `res` */
                           const uint8_t*  node_part,     /* same length: partition, < best_ploidy[block] */
                           const uint32_t* path_range,    /* [2*n_paths] inclusive SNP range, passed through */
                           uint32_t n_paths, floria_hip_haplosets** out);
int  floria_hip_reassign_haplosets_resident(floria_hip_ctx* ctx, const floria_hip_contig* const* contigs, uint32_t n_contigs,
                                            const floria_hip_haplosets* in, double epsilon, floria_hip_haplosets** out);

int  floria_hip_last_timing(const floria_hip_ctx* ctx, floria_timing* out);

/* Self-test of a hardware assumption: the beam kernel screens the pruning test (global_clustering.rs:98) with an f32 evaluation of stable_binom_cdf_p_rev
 * (utils_frags.rs:211-248) built on the hardware reciprocal and log2, and falls back to the exact host-libm table wherever the screen's error bound leaves a
 * decision open.  *max_err_per_n = max over n <= n_max, k <= n of |screen(n, k) - table(n, k)| / n on THIS device; the kernel assumes <= 2e-5. */
int  floria_hip_selftest(floria_hip_ctx* ctx, double epsilon, uint32_t n_max, double* max_err_per_n);

/* Tuning knob (0 = default): how many (block, ploidy) jobs may be resident at once. */
int  floria_hip_set_slots(floria_hip_ctx* ctx, uint32_t beam_slots);

/* The one option that selects WHICH function is computed: "arith".
 *   0 (default)  every weighted sum is carried as an exact (Q24 integer, number of epsilon terms) pair and rounded once;
 *   1            the reference's own arithmetic: running f64 sums, `diff += epsilon` between `diff += w` over a read's cells in the iteration order of its
 *                FxHashSet of positions (utils_frags.rs:33-72), one running sum per partition in a search node (global_clustering.rs:196-202), `errors +=`
 *                over a haplotype's positions in the bucket order of its FxHashMap (local_clustering.rs:226-256), those orders emulated on the device
 *                (csrc/arith_kernel.h; a pileup may instead CARRY its reads' set orders: floria_pileup::set_order, for fragments merged from several alignments).
 *                Applies to floria_hip_phase_* (S1) and floria_hip_reassign* (S2).  Every pileup - biallelic or not, with or without q = 0 cells - runs the
 *                shared-slab beam kernels with the running sums (beam_slab_kernel<.., ARITH>: terms folded per live slab; wide beams, ploidy * beam > 63:
 *                beam_wide_kernel<.., ARITH>, one lane per live slab, round 6); the optimise kernel lists a partition's position map in bucket order straight
 *                from the histogram where its keys span fewer positions than the map has buckets (every key then sits in its home bucket) and replays the
 *                insertions otherwise: about 1.5 x the time of mode 0 on BASELINE config 4 (97 against 66 ms at -e 0.04), 1.8 x on config 5; the host-pileup
 *                entry points pipeline in this mode too (every chunk's cell orders behind its flatten launch; two chunks by default).
 * For an epsilon that is a multiple of 2^-10 both modes return the same bits (every sum is exact in f64 in any order); for any other epsilon they are
 * different functions (about 60 % of the blocks of the BASELINE configs come out differently at 0.04) and mode 1 is the one a Rust host's CPU path computes,
 * as far as the emulated std hash-table orders are right.  Checked bit for bit against the oracle's arithmetic mode 1 (tests/test_gpu_arith.py).
 *
 * "s2_assign_only" = 1: floria_hip_reassign* stop behind the greedy re-insertion (part_block_manip.rs:203-222) and return the haplogroups as re-inserted —
 * input group order, input ranges, reads ascending — WITHOUT separate_broken_haplogroups (:27-98) and sort_parts (:276-288).  The read a split drops is the
 * first one behind a coverage gap in the iteration order of the reference's FxHashSet among reads that share a first_position; with the default (0) that
 * order is ascending counter_id, and which read goes changes the output of every short-read contig measured (scripts/a14_sensitivity.py; no long-read
 * one).  A Rust host that wants its own sets' order inserts the returned reads into its sets and keeps calling its own two functions: they are integer
 * bookkeeping, a few microseconds per contig.
 *
 * "s1_no_lists" = 1: floria_hip_phase_* leave the per-(block, read) lists on the device: read_id and part of the result are NULL (floria_hip_block_result_free copes),
 * every other field, the resident batch and the token are as before.  For a host that needs the lists on the device only (floria_hip_hap_graph,
 * floria_hip_join_paths): 5 B per (block, read) stay off the link.  Default 0: nothing changes.
 *
 * Tuning / test knobs; none changes results.  Keys: "groups" (job groups on separate streams, 0 = auto), "speculate" (ploidy stages: -1 auto,
 * 0 one ploidy at a time, 1 all ploidies of a block at once, 2 {1,2,3} then {4..P}), "spec_gate_div" (grid divisor of the gated ploidies of a
 * speculative stage, default 2), "tail_overlap" (one ploidy per stage: the beam launch of the LAST ploidy runs beside the optimise launch of the
 * ploidy below, every job waiting for its block's stop rule; 0 off = default (measured level with it on BASELINE config 4), 1 on), "tail_waves" (waves per CU of that launch,
 * default 2), "fuse_p1" (one ploidy per stage, canonical arithmetic, max_ploidy >= 2, ploidy-1 shortcut on: ploidy 1 gets no launches of its own, a block's ploidy-2
 * optimise job computes its MEC statistics and stop rule from the histogram it has built anyway; -1 auto = default = on where eligible, 0 off, 1 on where eligible;
 * FLORIA_HIP_FUSE_P1 in the environment), "beam_path" (0 auto, 1 generic, 2 slab, 3 wide), "no_specialized", "no_p1_shortcut", "opt_threads"
 * (0|128|512|1024), "opt_global", "opt_block_order" (tests / A/B: the optimise kernel's passes visit a block's reads in block order instead of longest first),
 * "opt_packed" (1 = default: the optimise kernel's build and distance passes stream one 4-byte packed cell per cell — SNP delta, allele, quality byte, weights from a table
 * in LDS — with 16-byte loads, where every contig of the call was uploaded through the library's flatten launch and the kernel is a ploidy-specialised instance; 0 = the
 * 8-byte cells everywhere; FLORIA_HIP_OPT_PACKED in the environment), "opt_delta" (1 = default: the 512-thread ploidy-specialised canonical instances of the optimise kernel keep a
 * read's distances as exact packed integers and, behind an accepted round, exchange only the terms at the code bytes that flipped, falling back to the interval pass
 * when more than 64 flipped or looking the cells up would cost more; 0 = f64 slots and the interval pass; FLORIA_HIP_OPT_DELTA in the environment; results are
 * bit for bit the same, floria_timing.optimize_delta_passes / optimize_delta_fallbacks say which pass ran), "slots", "stage_threads" (host threads that fill the pinned staging ring of a pageable upload),
 * "upload_chunks" (chunks of floria_hip_phase_pileups_batch, 0 = auto), "trace" (host-side timestamps of an S1 call on stderr), "reassign_path", "arith_hbm" (tests: the reference-arithmetic mode's tables in HBM scratch even where they fit into LDS), "arith_replay" (tests: that mode replays every position map insertion by insertion instead of listing it by the home-bucket rule where that applies), "fx_tags" / "arith_ow6" (A/B: size of the replay's claim table, the six-wave optimise instance at every ploidy), "no_bulk" (tests: every beam step through the general
 * insert path with its duplicate test), "asm_order_general" (tests: floria_hip_assemble_contigs_ordered sends every fragment through its one-thread-per-fragment
 * kernel; results do not change), "chain_wgs" (tests: N >= 1 = every grid-stride launch of the resident chain — the CIGAR walk, the realignment's gather and scatter,
 * assemble and its set orders, the FILL and ORDER passes of floria_hip_drop_monomorphic, the epilogue of floria_hip_reassign_batch_resident, floria_hip_join_paths, the device prologue of floria_hip_reassign_haplosets_resident — uses at most N workgroups, and the one-thread order kernel at most N threads,
 * so that a wavefront meets a second fragment, record or read at small inputs; 0 = default, the grids as they are; negative values are refused; results do not change), "inflate_slots" (tests: N >= 1 = floria_hip_inflate_bgzf keeps at most N members in flight, so that a wavefront of its persistent grid meets a second member; 0 = default, two per CU), "estimate_window" (tests: N = floria_hip_blob_estimate walks a group in windows of at most N positions, 1 .. 2^30; 0 = default, 2^22; results do not change), "hw_queues" (tests: override the number of
 * concurrently running streams floria_hip_create measured — 6 on an MI355X whose host set GPU_MAX_HW_QUEUES=12 before HIP initialised, 4 or fewer
 * with the runtime's default; below 5 the launch plans stay within two job groups and do not speculate). */
int  floria_hip_set_option(floria_hip_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* FLORIA_HIP_H */
