// inflate_core_check — the decoder core of csrc/inflate_kernel.h (the text the GPU runs) on the CPU, against zlib, under the sanitizers.
//   inflate_core_check CASES [N_CORRUPTIONS]
// CASES: one case per line, `name status isize hexpayload` (tests/inflate_cases.py).  Status 0: the output must equal what zlib inflates from the payload; any
// other status: the core must end with exactly it.  Then N_CORRUPTIONS seeded single-bit and single-byte corruptions of the valid cases: each must end with some
// status or with the right bytes (zlib's, when zlib still accepts the payload with that length), inside the step bound 8 x payload + isize.
// Every buffer is a heap allocation of the exact size, so an access the core's bounds let through is an AddressSanitizer report.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../floria_amd/csrc/inflate_kernel.h"

namespace {

struct HostIn {
    const uint8_t* p; uint32_t bytes; uint64_t max_word = 0;
    uint8_t byte(uint32_t i) const { return i < bytes ? p[i] : (uint8_t)0; }
    uint32_t word(uint32_t i) {
        if (i > max_word) max_word = i;
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint64_t o = 4ull * i + k; if (o < bytes) v |= (uint32_t)p[o] << (8 * k); }
        return v;
    }
};
struct HostOut {
    uint8_t* s;      // exactly out_bytes
    void put(uint32_t pos, uint8_t b) { s[pos] = b; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) s[pos + i] = s[pos - dist + (i < dist ? i : i % dist)]; }
    void copy_in(uint32_t pos, const HostIn& in, uint32_t off, uint32_t len) { for (uint32_t i = 0; i < len; ++i) s[pos + i] = in.byte(off + i); }
};
struct HostTab {
    uint16_t* t;     // exactly INF_TAB_WORDS
    uint16_t get(uint32_t i) const { return t[i]; }
    void set(uint32_t i, uint16_t v) { t[i] = v; }
};

struct Run { uint32_t status; uint64_t steps; std::vector<uint8_t> out; };

Run run_core(const std::vector<uint8_t>& payload, uint32_t isize) {
    uint8_t* in = new uint8_t[payload.size() ? payload.size() : 1];
    if (!payload.empty()) memcpy(in, payload.data(), payload.size());
    uint8_t* o = new uint8_t[isize ? isize : 1]();
    uint16_t* t = new uint16_t[fl::INF_TAB_WORDS]();
    HostIn hi{in, (uint32_t)payload.size()};
    HostOut ho{o};
    HostTab ht{t};
    Run r;
    r.status = fl::inflate_core(hi, hi.bytes, ho, isize, ht, &r.steps);
    if (hi.max_word > payload.size() / 4 + 3) { fprintf(stderr, "the core asked for payload word %llu of a %zu-byte payload\n", (unsigned long long)hi.max_word, payload.size()); exit(3); }
    r.out.assign(o, o + isize);
    delete[] in; delete[] o; delete[] t;
    return r;
}

// zlib's raw inflate: true and the bytes when the payload is a complete stream
bool zlib_inflate(const std::vector<uint8_t>& payload, std::vector<uint8_t>& out) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) { fprintf(stderr, "inflateInit2 failed\n"); exit(3); }
    out.assign(70000, 0);
    static uint8_t none[1];
    z.next_in = payload.empty() ? none : const_cast<uint8_t*>(payload.data()); z.avail_in = (uInt)payload.size();
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END;
    out.resize(ok ? z.total_out : 0);
    inflateEnd(&z);
    return ok;
}

struct Case { std::string name; uint32_t status, isize; std::vector<uint8_t> payload; };

uint64_t rng_state = 0x1577f10a1aull;
uint64_t rnd() { uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: inflate_core_check CASES [N_CORRUPTIONS]\n"); return 2; }
    const int n_corrupt = argc > 2 ? atoi(argv[2]) : 2000;
    std::ifstream f(argv[1]);
    std::vector<Case> cases;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        Case c; std::string hex;
        if (!(ss >> c.name >> c.status >> c.isize >> hex)) continue;
        if (hex != "-") for (size_t i = 0; i + 1 < hex.size(); i += 2) c.payload.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
        cases.push_back(c);
    }
    if (cases.empty()) { fprintf(stderr, "no cases in %s\n", argv[1]); return 2; }
    int bad = 0;
    std::vector<const Case*> valid;
    for (const Case& c : cases) {
        const Run r = run_core(c.payload, c.isize);
        const uint64_t bound = 8ull * c.payload.size() + c.isize;
        bool ok = r.status == c.status && r.steps <= bound;
        if (c.status == 0) {
            std::vector<uint8_t> want;
            ok = ok && zlib_inflate(c.payload, want) && want.size() == c.isize && want == r.out;
            valid.push_back(&c);
        }
        printf("%-34s status %2u (want %2u) steps %8llu of %8llu  %s\n", c.name.c_str(), r.status, c.status, (unsigned long long)r.steps, (unsigned long long)bound, ok ? "ok" : "FAILED");
        bad += !ok;
    }
    int n_status = 0, n_same = 0;
    for (int k = 0; k < n_corrupt && !valid.empty(); ++k) {
        const Case& c = *valid[rnd() % valid.size()];
        if (c.payload.empty()) continue;
        std::vector<uint8_t> p = c.payload;
        const size_t at = rnd() % p.size();
        if (k & 1) p[at] ^= (uint8_t)(1u << (rnd() % 8)); else p[at] = (uint8_t)rnd();
        const Run r = run_core(p, c.isize);
        const uint64_t bound = 8ull * p.size() + c.isize;
        bool ok = r.steps <= bound && r.status < fl::INF_N_STATUS && r.status != fl::INF_STEPS;
        if (r.status == 0) {
            std::vector<uint8_t> want;
            ok = ok && zlib_inflate(p, want) && want.size() == c.isize && want == r.out;
            ++n_same;
        } else ++n_status;
        if (!ok) { printf("corruption %d of %s at byte %zu: status %u, %llu steps of %llu  FAILED\n", k, c.name.c_str(), at, r.status, (unsigned long long)r.steps, (unsigned long long)bound); ++bad; }
    }
    printf("%d corruptions: %d ended with a status, %d with zlib's bytes\n", n_corrupt, n_status, n_same);
    printf(bad ? "%d FAILED\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
