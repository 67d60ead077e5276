#!/usr/bin/env python
"""(GPU) Rate of the fixed-block walk kernel (realign_walk_kernel.h) per step against the exact kernel (realign_kernel.h) on the same windows in the same process,
alternating, device events around every launch (scripts/probes/realign_walk_bench.hip, compiled here if it is missing), in windows / s and computed DP cells / s.
Cells per alignment: the exact DP computes 33 x 33; a walk's count is the definition's `cells_out`, taken here from synth_bam.walk_affine_batch(want_cells=True)
(pinned to scripts/probes/block_walk.c by tests/test_realign_walk_cpu.py) on a sample of the windows.
usage: scripts/realign_walk_bench.py [windows = 2000000] [seconds = 0.5]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floria_amd import synth_bam  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
exe = os.path.join(ROOT, "scripts", "probes", "realign_walk_bench")
if not os.path.exists(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "floria_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", exe, exe + ".hip"])
rng = np.random.default_rng(1)
B = np.frombuffer(b"ACGT", np.uint8)
r = B[rng.integers(0, 4, size=(n, 32))]
q = r.copy()
m = rng.random((n, 32)) < 0.10                       # 10 % substitutions; neither kernel's work depends on the bases
q[m] = B[rng.integers(0, 4, size=int(m.sum()))]
al = np.zeros((n, 4), np.uint8); al[:, 0] = r[:, 16]; al[:, 1] = B[(np.searchsorted(B, al[:, 0]) + 1) % 4]
na = np.full(n, 2, np.uint8)
cells = {"exact": 33 * 33}
for step in (1, 2, 4, 8):
    c = synth_bam.walk_affine_batch(q[:200], r[:200], step, 0, 0, want_cells=True)[1]
    assert c.min() == c.max()
    cells[f"walk step {step}"] = int(c[0])
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "windows.bin")
    with open(path, "wb") as f:
        for a in (q, r, al, na):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, path, str(n), str(seconds)], capture_output=True, text=True)
if out.returncode:
    print(out.stderr)
    raise SystemExit(out.returncode)
print(f"# {n} windows, 2 alleles each; device events around every launch, kernels alternating, >= {seconds} s of device time each after one warm-up launch")
for line in out.stdout.splitlines():
    name, launches, ms, wps = line.split("\t")
    print(f"{name:12s} {int(launches):4d} launches {float(ms):9.1f} ms  {float(wps) / 1e6:8.2f} M windows/s  {cells[name]:5d} cells per alignment  "
          f"{float(wps) * 2 * cells[name] / 1e12:6.3f} T cells/s")
