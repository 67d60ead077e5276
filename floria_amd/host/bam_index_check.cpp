// bam_index_check — BamStream, the .bai reader and the record decode of ingest.cpp on their own, for a memory-safety build (make bam-index-check-asan:
// -fsanitize=address,undefined).  Plain host code: it links no device library; the entry points of the C ABI that ingest.cpp names elsewhere are defined
// in bam_index_check_stubs.cpp to abort, none is reached from this program.
//
//   bam_index_check FILE.bam [--no-index] [--window BYTES] [--threads N] [--select TID ...]
//
// Streams the file (through the index beside it unless --no-index; --select narrows to those targets, as the driver does after reading the VCF) and prints per
// segment its target range and per target its records and a sum over every decoded field of each, then the index use.  Exit 0; 3 with the message when the
// library refuses the input (floria::Error), which is the expected end for a malformed index.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "floria_host.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { fputs("usage: bam_index_check FILE.bam [--no-index] [--window BYTES] [--threads N] [--select TID ...]\n", stderr); return 2; }
    bool use_index = true, selecting = false;
    size_t window = 1 << 20, threads = 2;
    std::vector<int32_t> tids;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--no-index") use_index = false;
        else if (a == "--window" && i + 1 < argc) window = (size_t)strtoull(argv[++i], nullptr, 10);
        else if (a == "--threads" && i + 1 < argc) threads = (size_t)strtoull(argv[++i], nullptr, 10);
        else if (a == "--select") { selecting = true; while (i + 1 < argc && argv[i + 1][0] != '-') tids.push_back((int32_t)atoi(argv[++i])); }
        else { fprintf(stderr, "bam_index_check: unknown argument %s\n", a.c_str()); return 2; }
    }
    try {
        floria::BamStream stream(argv[1], threads, use_index);
        if (selecting) stream.select(tids);
        floria::BamFile seg;
        while (stream.next(seg, window)) {
            printf("segment [%d, %d): %zu records\n", seg.tid_begin, seg.tid_end, seg.records.size());
            for (int32_t t = seg.tid_begin; t < seg.tid_end; ++t) {
                if (seg.by_tid[(size_t)t].empty()) continue;
                uint64_t sum = 0;
                for (uint32_t ix : seg.by_tid[(size_t)t]) {
                    const floria::BamRecord& r = seg.records[ix];
                    sum = sum * 1099511628211ull + (uint64_t)(uint32_t)r.tid + ((uint64_t)(uint32_t)r.pos << 20) + r.flags + ((uint64_t)r.mapq << 50);
                    for (char c : r.qname) sum = sum * 31 + (unsigned char)c;
                    for (size_t k = 0; k < r.cigar.size(); ++k) sum = sum * 31 + r.cigar[k];
                    for (size_t k = 0; k < r.seq.size(); ++k) sum = sum * 31 + (unsigned char)r.seq[k];
                    for (size_t k = 0; k < r.qual.size(); ++k) sum = sum * 31 + r.qual[k];
                }
                printf("target %d: %zu records, sum %016llx\n", t, seg.by_tid[(size_t)t].size(), (unsigned long long)sum);
            }
        }
        if (!stream.index_path().empty()) {
            const floria::BamStream::IndexUse u = stream.index_use();
            printf("index %s: %zu selected, %zu members inflated of %zu\n", stream.index_path().c_str(), u.selected, u.members_inflated, u.members_in_file);
        }
        printf("peak buffer %zu bytes\n", stream.peak_buffer_bytes());
    } catch (const floria::Error& e) {
        printf("refused: %s\n", e.what());
        return 3;
    }
    return 0;
}
