"""`-m gpu`: a plain bench.py run (the headline only) and its --dump-outputs: the files hold what the last timed step computed,
checked block for block against the CPU oracle on the same seeded contigs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTIGS = 12


def test_plain_run_times_the_steps_and_dumps_what_they_computed(hip_lib, oracle_mod, tmp_path):
    from floria_amd import synth
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--contigs", str(CONTIGS),
                        "--dump-outputs", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value_is"] == "resident" and d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["total_blocks"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for leg in ("cpu_baseline", "second_pass", "spot_check", "pipeline"):          # --full only
        assert not d.get(leg), leg
    assert d["value_h2d_inclusive"] is None

    a = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
    C = synth.CONFIGS[4]
    blocks = []
    for gid in range(CONTIGS):
        c = synth.make_config_contig(4, gid)
        s, e = hip_lib.get_range_with_lengths(c.snp_pos, C["block_length"])
        ro = oracle_mod.phase_blocks(c.pileup, s, e, oracle_mod.make_params(0.03125, C["max_ploidy"], C["beam"]), threads=4)
        for k in range(len(s)):
            lo, hi = int(ro.read_off[k]), int(ro.read_off[k + 1])
            blocks.append((ro.best_ploidy[k], ro.ploidies_tried[k], ro.mec[k], ro.read_id[lo:hi], ro.part[lo:hi]))
    nb = len(blocks)
    assert nb == d["config"]["total_blocks"] and a["best_ploidy"].shape == (nb,) and a["mec"].shape == (nb, C["max_ploidy"])
    assert np.array_equal(a["best_ploidy"], [b[0] for b in blocks]) and np.array_equal(a["ploidies_tried"], [b[1] for b in blocks])
    assert np.array_equal(a["mec"].view(np.uint64), np.array([b[2] for b in blocks], np.float64).view(np.uint64))
    assert np.array_equal(a["reads_per_block"], [len(b[3]) for b in blocks])
    pick = a["sample_blocks"].astype(np.int64)
    assert len(pick) == nb                                       # a small job: every block is in the sample
    assert np.array_equal(a["sample_read_id"], np.concatenate([blocks[b][3] for b in pick]))
    assert np.array_equal(a["sample_part"], np.concatenate([blocks[b][4] for b in pick]))
