// The packed cell of the optimise kernel's 4-byte stream (floria_amd/csrc/common.h): pack / unpack round trips over the extremes, and the weight table the
// packed-cell instances stage in LDS against phred_scale (utils_frags.rs:702-711) and against what flatten_kernel folds into cell_aw.  Host code only; built
// with -fsanitize=address,undefined by tests/test_packed_cells_cpu.py.
#include "common.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad < 20) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad; } } while (0)

int main() {
    using namespace fl;
    // ---- the table ----------------------------------------------------------------------------------------------------------------
    std::vector<uint32_t> w(256);
    CHECK(w24_table(w.data()), "some weight is not a multiple of 2^-24");
    for (int q = 0; q < 256; ++q) {
        const float prob = 1.0f - std::pow(10.0f, (float)q / -10.0f);          // the reference's f32 expression
        const double s = std::ldexp((double)prob, 24);
        CHECK(s == std::floor(s) && s >= 0.0 && s <= 16777216.0, "q = %d: %.17g", q, s);
        CHECK((double)w[q] == s, "q = %d: table %u, phred_scale %.17g", q, w[q], s);
        CHECK(w[q] <= ONE_Q24, "q = %d", q);
        if (q) CHECK(w[q] >= w[q - 1], "q = %d: not monotone", q);
        // (the weight saturates where 10^(-q/10) falls below half an f32 ulp of 1, 2^-25: from q = 76 on; q = 73..75 still give 2^24 - 1)
        CHECK((w[q] == ONE_Q24) == (std::pow(10.0, q / -10.0) < std::ldexp(1.0, -25)), "q = %d: weight %u", q, w[q]);
    }
    CHECK(w[0] == 0 && w[72] < ONE_Q24 && w[75] == ONE_Q24 - 1 && w[76] == ONE_Q24 && w[255] == ONE_Q24, "weights at q = 0, 72, 75, 76, 255: %u %u %u %u %u", w[0], w[72], w[75], w[76], w[255]);
    // ---- round trips: deltas at both ends and around every power of two, alleles 0-3, every quality byte -------------------------------------
    std::vector<uint32_t> deltas = {0u, 1u, 2u, PK_DELTA_MAX - 1u, PK_DELTA_MAX};
    for (uint32_t b = 1; b < PK_DELTA_BITS; ++b) { deltas.push_back((1u << b) - 1u); deltas.push_back(1u << b); deltas.push_back((1u << b) + 1u); }
    unsigned long long n = 0;
    for (uint32_t d : deltas) {
        CHECK(pk_fits(d), "delta %u", d);
        for (uint32_t a = 0; a < 4; ++a)
            for (uint32_t q = 0; q < 256; ++q) {
                const uint32_t pk = pk_pack(d, a, q);
                CHECK(pk_delta(pk) == d && pk_allele(pk) == a && pk_qual(pk) == q, "delta %u allele %u qual %u -> %08x -> %u %u %u", d, a, q, pk, pk_delta(pk), pk_allele(pk), pk_qual(pk));
                CHECK(pk_to_aw(pk, w.data()) == ((a << 28) | w[q]), "delta %u allele %u qual %u: cell_aw %08x", d, a, q, pk_to_aw(pk, w.data()));
                ++n;
            }
    }
    // distinct cells pack to distinct words (the fields do not overlap)
    CHECK(pk_pack(1, 0, 0) != pk_pack(0, 1, 0) && pk_pack(0, 1, 0) != pk_pack(0, 0, 1) && pk_pack(0, 3, 255) < pk_pack(1, 0, 0), "fields overlap");
    // what does not fit says so
    CHECK(!pk_fits(PK_DELTA_MAX + 1u) && !pk_fits(0xffffffffu) && PK_DELTA_MAX == (1u << 20) - 1u, "pk_fits");
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("packed_cell_test: %llu round trips, 256 weights: ok\n", n);
    return 0;
}
