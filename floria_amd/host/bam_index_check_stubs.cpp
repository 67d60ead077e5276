// The entry points of libfloria_hip.so that ingest.cpp names in its device routes, for bam_index_check, which links no device library and reaches none of them.
// (No header of the project is included: these are stand-ins by name only.)
#include <cstdio>
#include <cstdlib>

#define DEVICE_ENTRY(name) extern "C" int name(...) { fprintf(stderr, "bam_index_check: device entry point " #name " reached\n"); abort(); }
DEVICE_ENTRY(floria_hip_assemble_contigs_opt)
DEVICE_ENTRY(floria_hip_blob_bytes)
DEVICE_ENTRY(floria_hip_blob_download)
DEVICE_ENTRY(floria_hip_blob_estimate)
DEVICE_ENTRY(floria_hip_blob_free)
DEVICE_ENTRY(floria_hip_blob_records_free)
DEVICE_ENTRY(floria_hip_blob_records_opt)
DEVICE_ENTRY(floria_hip_blob_sequences)
DEVICE_ENTRY(floria_hip_blob_sequences_free)
DEVICE_ENTRY(floria_hip_inflate_bgzf)
DEVICE_ENTRY(floria_hip_pileup_records_resident_blob)
DEVICE_ENTRY(floria_hip_contig_free)
DEVICE_ENTRY(floria_hip_drop_monomorphic)
DEVICE_ENTRY(floria_hip_estimate_result_free)
DEVICE_ENTRY(floria_hip_last_timing)
DEVICE_ENTRY(floria_hip_mono_result_free)
DEVICE_ENTRY(floria_hip_pileup_records)
DEVICE_ENTRY(floria_hip_pileup_records_realign)
DEVICE_ENTRY(floria_hip_pileup_records_resident)
DEVICE_ENTRY(floria_hip_record_cells_free)
DEVICE_ENTRY(floria_hip_record_summary_free)
extern "C" const char* floria_hip_last_error(void) { return "no device library in bam_index_check"; }
