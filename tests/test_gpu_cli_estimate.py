"""`-m gpu`: floria-hip --pileup resident --inflate device --estimate device without -e / -l against --estimate host: the `Estimated` line, cmd.log (its first line
is the command line, so the flag's own value is put back before the comparison) and every file byte for byte; --dump-estimate of both routes; the report line."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from floria_amd import synth_bam
from tests import plan_model as plm
from tests.test_gpu_cli_resident import HAND, NINE, floria_hip, nine, noisy, paired  # noqa: F401 (fixtures)
from tests.test_gpu_pileup import hand_built

pytestmark = pytest.mark.gpu

REPORT = re.compile(r"Estimate on the device: (\d+) of those segments read by the -e / -l estimate in ([0-9.]+)s \((\d+) floria_hip_blob_estimate calls; device events: upload ([0-9.]+)s, "
                    r"kernels ([0-9.]+)s, download ([0-9.]+)s\)")


def run(floria_hip, prefix, out, estimate, extra=(), ingest_only=False):
    if os.path.exists(out):
        shutil.rmtree(out)
    cmd = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", out, "-t", "4", "--pileup", "resident", "--inflate", "device", "--estimate", estimate, *extra]
    r = subprocess.run(cmd + (["--ingest-only"] if ingest_only else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    tree = {}
    for dp, _, fs in os.walk(out):
        for f in fs:
            tree[os.path.relpath(os.path.join(dp, f), out)] = open(os.path.join(dp, f), "rb").read()
    return tree, r.stderr


def estimate_agrees(floria_hip, tmp_path, prefix, extra=(), min_files=4):
    out = str(tmp_path / "out")
    host_tree, host_err = run(floria_hip, prefix, out, "host", extra)
    dev_tree, dev_err = run(floria_hip, prefix, out, "device", extra)
    line = lambda err: re.search(r"Estimated -l \d+, -e \S+ \(used where not given: [^)]*\)", err).group(0)
    assert line(dev_err) == line(host_err)
    assert sorted(dev_tree) == sorted(host_tree) and len(host_tree) >= min_files and "cmd.log" in host_tree
    dev_tree["cmd.log"] = dev_tree["cmd.log"].replace(b"--estimate device ", b"--estimate host ", 1)
    for fn in host_tree:
        assert dev_tree[fn] == host_tree[fn], f"{fn} differs"
    m = REPORT.search(dev_err)
    assert m and int(m.group(1)) >= 1 and int(m.group(3)) == int(m.group(1)), dev_err
    assert "Estimate on the device:" not in host_err
    return host_err, dev_err, m


def dumps_agree(floria_hip, tmp_path, prefix, extra=()):
    dumps = {}
    for estimate in ("host", "device"):
        f = str(tmp_path / f"estimate_{estimate}.txt")
        run(floria_hip, prefix, str(tmp_path / "unused"), estimate, (*extra, "--dump-estimate", f), ingest_only=True)
        dumps[estimate] = open(f).read()
    assert dumps["host"] == dumps["device"] and "\ncount " in dumps["host"] and "\nlength " in dumps["host"]
    return dumps["host"]


def test_noisy_long_reads(floria_hip, tmp_path, noisy):
    estimate_agrees(floria_hip, tmp_path, noisy)
    host_err, _, _ = estimate_agrees(floria_hip, tmp_path, noisy, extra=("--epsilon-round",))      # cmd.log then carries the estimated -e on a second line
    assert "Estimated -l" in host_err
    dump = dumps_agree(floria_hip, tmp_path, noisy)
    assert len(dump.splitlines()) > 10


def test_paired_short_reads(floria_hip, tmp_path, paired):
    estimate_agrees(floria_hip, tmp_path, paired)
    dumps_agree(floria_hip, tmp_path, paired)


def test_flag_is_unused_where_both_parameters_are_given(floria_hip, tmp_path, paired):
    _, err = run(floria_hip, paired, str(tmp_path / "out"), "device", ("-e", "0.04", "-l", "500"))
    assert "Estimated" not in err and "Estimate on the device:" not in err and "Inflate on the device:" in err


def test_record_whose_cigar_lives_in_the_cg_tag(floria_hip, tmp_path):
    """the CG record of tests/test_gpu_cli_inflate.py, shorter: 4 000 x (1M 1I) behind the kSmN placeholder; the estimate walks the CG array where it lies in the blob"""
    prefix = str(tmp_path / "cg")
    hand_built(prefix)
    targets, records = plm.read_bam(prefix + ".bam")
    at, n = 9000, 4000
    seq = np.frombuffer(b"ACGT" * (n // 2), np.uint8)
    rec = synth_bam.bam_record(0, at, "x_cg", 0, 60, [("S", 2 * n), ("N", n)], bytes(seq), np.full(2 * n, 30, np.uint8))
    cigar = b"".join(struct.pack("<II", 1 << 4 | 0, 1 << 4 | 1) for _ in range(n))
    body = rec[4:] + b"XAA!" + b"CGBI" + struct.pack("<I", 2 * n) + cigar
    rows = sorted([(r["pos"], r["raw"]) for r in records] + [(at, struct.pack("<I", len(body)) + body)], key=lambda t: t[0])
    synth_bam.write_bam(prefix + ".bam", targets, [raw for _, raw in rows])
    estimate_agrees(floria_hip, tmp_path, prefix, extra=HAND)
    dump = dumps_agree(floria_hip, tmp_path, prefix, extra=HAND)
    assert f"length {2 * n} " in dump                                     # the CG record gave bases to sampled columns


def test_a_small_window_makes_the_pass_read_several_segments(floria_hip, tmp_path, nine):
    extra = (*NINE, "--bam-window-kb", "64")
    _, _, m = estimate_agrees(floria_hip, tmp_path, nine, extra=extra, min_files=30)
    assert int(m.group(1)) >= 3
    assert dumps_agree(floria_hip, tmp_path, nine, extra=extra) == dumps_agree(floria_hip, tmp_path, nine, extra=NINE)
