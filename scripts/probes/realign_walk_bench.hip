// Rate of realign_walk_kernel (every step; rule max, tie right — the rule and the tie do not change the amount of work) against realign_kernel on the SAME windows in the
// same process, the two alternating, device events around each launch, until each has at least `seconds` of device time after a warm-up launch.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I floria_amd/csrc -I include -o scripts/probes/realign_walk_bench scripts/probes/realign_walk_bench.hip
//   scripts/probes/realign_walk_bench windows.bin N [seconds = 0.5]      windows.bin: N x (32 read bases, 32 reference bases, 4 alleles, 1 n_alleles) as four arrays
// Prints one line per kernel: name, launches, milliseconds, windows / s.  (scripts/realign_walk_bench.py writes the windows and turns the lines into cells / s.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "floria_hip.h"
#include "realign_walk_kernel.h"

#define CHK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

template <class K> static int timed(K kern, uint32_t grid, const fl::RealignArgs& a, hipEvent_t e0, hipEvent_t e1, float* ms) {
    CHK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, a);
    CHK(hipGetLastError());
    CHK(hipEventRecord(e1, 0));
    CHK(hipEventSynchronize(e1));
    CHK(hipEventElapsedTime(ms, e0, e1));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: realign_walk_bench windows.bin N [seconds]\n"); return 2; }
    const size_t n = strtoull(argv[2], nullptr, 10);
    const double want_ms = 1e3 * (argc > 3 ? atof(argv[3]) : 0.5);
    std::vector<uint8_t> host(n * 69);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(host.data(), 1, host.size(), f) != host.size()) { fprintf(stderr, "cannot read %zu bytes from %s\n", host.size(), argv[1]); return 2; }
    fclose(f);
    uint8_t* d = nullptr; uint8_t* best = nullptr;
    CHK(hipMalloc((void**)&d, host.size())); CHK(hipMalloc((void**)&best, n));
    CHK(hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice));
    fl::RealignArgs a{};
    a.q = d; a.r = d + 32 * n; a.alleles = d + 64 * n; a.n_alleles = d + 68 * n; a.best = best; a.score = nullptr; a.n = n;
    hipDeviceProp_t prop; CHK(hipGetDeviceProperties(&prop, 0));
    const uint32_t cus = (uint32_t)prop.multiProcessorCount;
    const uint32_t grid_exact = (uint32_t)std::min<uint64_t>((n + 3) / 4, (uint64_t)cus * 32), grid_walk = (uint32_t)std::min<uint64_t>((n + 15) / 16, (uint64_t)cus * 32);   // as floria_hip.hip launches them
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    double ms[5] = {0, 0, 0, 0, 0}; int launches[5] = {0, 0, 0, 0, 0};
    const char* name[5] = {"exact", "walk step 1", "walk step 2", "walk step 4", "walk step 8"};
    for (int round = 0; ; ++round) {                       // round 0 = warm-up, not counted
        bool more = round <= 1;
        for (int k = 0; k < 5; ++k) {
            if (round > 1 && ms[k] >= want_ms) continue;
            float t = 0;
            int rc = k == 0 ? timed(fl::realign_kernel, grid_exact, a, e0, e1, &t) : k == 1 ? timed(fl::realign_walk_kernel<1, 0, 0>, grid_walk, a, e0, e1, &t)
                   : k == 2 ? timed(fl::realign_walk_kernel<2, 0, 0>, grid_walk, a, e0, e1, &t) : k == 3 ? timed(fl::realign_walk_kernel<4, 0, 0>, grid_walk, a, e0, e1, &t)
                            : timed(fl::realign_walk_kernel<8, 0, 0>, grid_walk, a, e0, e1, &t);
            if (rc) return rc;
            if (round > 0) { ms[k] += t; ++launches[k]; if (ms[k] < want_ms) more = true; }
        }
        if (!more || round > 100000) break;
    }
    for (int k = 0; k < 5; ++k) printf("%s\t%d\t%.3f\t%.0f\n", name[k], launches[k], ms[k], (double)n * launches[k] / (ms[k] * 1e-3));
    CHK(hipFree(d)); CHK(hipFree(best));
    return 0;
}
