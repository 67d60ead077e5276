"""`-m "not gpu"`: the column model of the -e / -l estimate (tests/estimate_model.py) pinned to the C++ host's pass (floria-hip --ingest-only --dump-estimate, which
needs no device on the host route) and to l_epsilon_restated of tests/test_host_cpu.py; the refusals and usage text of --estimate; the symbol, struct and sketch
entries of floria_hip_blob_estimate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from floria_amd import _capi as capi
from floria_amd import synth, synth_bam
from tests import estimate_model as model
from tests import plan_model as plm
from tests.test_host_cpu import l_epsilon_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
OPS = "MIDNSHP=X"


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def bam_groups(path):
    """the BAM's records as the estimate takes them: filtered, one group per target in header order, ascending by pos -> (groups, tid of every group)"""
    targets, records = plm.read_bam(path)
    code = {c: k for k, c in enumerate(plm.NT16)}
    by_tid = {}
    for r in records:
        if r["tid"] < 0 or r["flag"] & 1796 or not r["cigar"]:
            continue
        by_tid.setdefault(r["tid"], []).append((r["pos"], [(OPS.index(op), n) for op, n in r["cigar"]], np.array([code[b] for b in r["seq"]], np.int64)))
    tids = sorted(by_tid)
    return [sorted(by_tid[t], key=lambda r: r[0]) for t in tids], tids


def parse_dump(path):
    cols, lengths, state = [], [], {}
    for line in open(path):
        f = line.split()
        if f[0] == "length":
            lengths.append((int(f[1]), int(f[2])))
        elif f[0] in ("count", "n_err"):
            state[f[0]] = int(f[1])
        else:
            cols.append(tuple(map(int, f)))
    return cols, lengths, state


def dump_estimate(floria_hip, prefix, tmp_path, extra=()):
    out = str(tmp_path / "estimate.txt")
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "--ingest-only", "--dump-estimate", out, *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Estimated -l (\d+), -e (\S+) ", r.stderr)
    return parse_dump(out), (int(m.group(1)), m.group(2))


def against_the_host(floria_hip, prefix, tmp_path, extra=()):
    (cols, lengths, state), (l, e) = dump_estimate(floria_hip, prefix, tmp_path, extra)
    groups, tids = bam_groups(prefix + ".bam")
    want = model.estimate(groups, 1000)
    assert cols == [(tids[g], p, t, m) for g, p, t, m in want["cols"]]
    assert state == dict(count=want["count"], n_err=want["n_err"]) and lengths == model.lengths_of(groups, want["rec_hits"])
    wl, we = model.result(want["cols"], lengths)
    assert l == wl and e == "%g" % we
    return want


def add_records(prefix, extra):
    """the data set's BAM with hand-built records (tid, pos, cigar, flag) added: bases random, qualities 30"""
    targets, records = plm.read_bam(prefix + ".bam")
    rng = np.random.default_rng(4)
    rows = [(r["tid"], r["pos"], r["raw"]) for r in records]
    for k, (tid, pos, cigar, flag) in enumerate(extra):
        n = sum(ln for op, ln in cigar if op in "MIS=X")
        rows.append((tid, pos, synth_bam.bam_record(tid, pos, f"extra{k}", flag, 60, cigar, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)), np.full(n, 30, np.uint8))))
    rows.sort(key=lambda t: (t[0], t[1]))
    synth_bam.write_bam(prefix + ".bam", targets, [raw for _, _, raw in rows])


def test_long_reads_with_indels_soft_clips_and_a_hard_clipped_supplementary_piece(floria_hip, tmp_path):
    c = synth.make_config_contig(4, 1, keep_layout=True)
    prefix = str(tmp_path / "long")
    synth_bam.write_dataset(prefix, [c], seed=3, edit_frac=0.5, realign=False)
    add_records(prefix, [(0, 0, [("S", 7), ("M", 400), ("I", 3), ("M", 200), ("D", 5), ("=", 100), ("X", 2), ("M", 900), ("S", 11)], 0),
                         (0, 1, [("H", 300), ("M", 700), ("N", 40), ("M", 300), ("H", 20)], 2048),
                         (0, 2, [("M", 500)], 256), (0, 3, [("M", 500)], 1024), (0, 5, [("M", 500)], 4)])      # the last three are filtered
    want = against_the_host(floria_hip, prefix, tmp_path, ("--no-realign",))
    assert want["n_err"] >= 3


def test_paired_short_reads(floria_hip, tmp_path):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path / "paired")
    synth_bam.write_dataset(prefix, [c], seed=7)
    want = against_the_host(floria_hip, prefix, tmp_path)
    assert len(model.lengths_of(*[bam_groups(prefix + ".bam")[0]], want["rec_hits"])) >= 1


def test_two_contigs_and_a_gap_between_the_reads_of_one(floria_hip, tmp_path):
    cs = [synth.make_config_contig(4, 20, 0.12, keep_layout=True), synth.make_config_contig(4, 21, 0.14, keep_layout=True)]
    prefix = str(tmp_path / "two")
    synth_bam.write_dataset(prefix, cs, seed=7, edit_frac=0.5, realign=False)
    targets, records = plm.read_bam(prefix + ".bam")
    # cut a hole of 3 000 positions into the first contig's coverage: every record of it that begins in [4 000, 9 000) goes
    kept = [r["raw"] for r in records if not (r["tid"] == 0 and 4000 <= r["pos"] < 9000)]
    assert len(kept) < len(records)
    synth_bam.write_bam(prefix + ".bam", targets, kept)
    want = against_the_host(floria_hip, prefix, tmp_path, ("--no-realign",))
    assert {g for g, *_ in want["cols"]} == {0, 1}


def test_the_model_is_the_restatement_on_gapless_input(tmp_path):
    c = synth.make_config_contig(4, 1, keep_layout=True)
    ex = synth_bam.write_dataset(str(tmp_path / "d"), [c], seed=2, edit_frac=0.0, realign=False)[c.name]
    code = {c: k for k, c in enumerate(plm.NT16)}
    as_bytes = lambda s: s.encode() if isinstance(s, str) else bytes(s)
    recs = sorted(((int(a[0]), [(0, len(a[1]))], np.array([code[b] for b in as_bytes(a[1])], np.int64)) for a in ex["alignments"]), key=lambda r: r[0])
    got = model.estimate([recs], 1000)
    assert model.result(got["cols"], model.lengths_of([recs], got["rec_hits"])) == l_epsilon_restated(ex["alignments"])


# ---- the flag ------------------------------------------------------------------------------------------------------------------------------------------
def run(floria_hip, *args):
    return subprocess.run([floria_hip, "-b", "none.bam", "-v", "none.vcf", "-r", "none.fa", *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("route", [(), ("--inflate", "host", "--pileup", "resident"), ("--pileup", "host")])
def test_estimate_device_without_inflate_device_is_refused_with_the_reason(floria_hip, route):
    r = run(floria_hip, "--estimate", "device", *route)
    assert r.returncode == 1 and "--estimate device needs --inflate device: the estimate then reads the blobs that route inflates on the device" in r.stderr


def test_estimate_takes_host_or_device(floria_hip):
    r = run(floria_hip, "--estimate", "bogus")
    assert r.returncode == 1 and "--estimate takes host or device, not 'bogus'" in r.stderr
    r = run(floria_hip, "--estimate")
    assert r.returncode == 1 and "missing value for --estimate" in r.stderr
    for extra in (("--estimate", "host"), ("--estimate", "host", "--pileup", "device"), ("--estimate", "device", "--inflate", "device", "--pileup", "resident"),
                  ("--estimate", "device", "--inflate", "device", "--pileup", "resident", "-e", "0.04", "-l", "1000")):
        r = run(floria_hip, *extra)
        assert r.returncode == 1 and "cannot open none.bam" in r.stderr and "--estimate" not in r.stderr
    r = run(floria_hip, "--dump-estimate", "x.txt")
    assert r.returncode == 1 and "--dump-estimate needs --ingest-only" in r.stderr
    r = run(floria_hip, "--dump-estimate", "x.txt", "--ingest-only", "-e", "0.04", "-l", "1000")
    assert r.returncode == 1 and "--dump-estimate needs the estimate" in r.stderr


def test_help_names_the_flag(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--estimate host|device" in r.stderr and "floria_hip_blob_estimate" in r.stderr and "Needs --inflate device" in r.stderr


# ---- the library boundary --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_structs_and_the_sketch(hip_lib):
    L = hip_lib.load()
    sketch = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "floria_hip.h")).read()
    stubs = open(os.path.join(HOST, "bam_index_check_stubs.cpp")).read()
    for s in ("floria_hip_blob_estimate", "floria_hip_estimate_result_free"):
        assert s in hip_lib.SYMBOLS and hasattr(L, s) and "pub fn " + s + "(" in sketch and s + "(" in header and f"DEVICE_ENTRY({s})" in stubs, s
    assert [f for f, _ in capi.CEstimateRecords._fields_] == ["n", "pos", "cigar_off", "n_cigar", "seq_off", "l_seq", "n_groups", "group_off"] and C.sizeof(capi.CEstimateRecords) == 64
    assert [f for f, _ in capi.CEstimateState._fields_] == ["count", "n_err"] and C.sizeof(capi.CEstimateState) == 16
    assert [f for f, _ in capi.CEstimateResult._fields_] == ["n_cols", "col_group", "col_pos", "col_total", "col_most", "rec_hits", "done"] and C.sizeof(capi.CEstimateResult) == 56
    for s in ("pub struct FloriaEstimateRecords", "pub struct FloriaEstimateState", "pub struct FloriaEstimateResult"):
        assert s in sketch, s
    assert hasattr(hip_lib.FloriaHip, "blob_estimate")


def test_null_arguments_are_refused_without_a_device(hip_lib):
    L = hip_lib.load()
    out = C.POINTER(capi.CEstimateResult)()
    state = capi.CEstimateState(0, 0)
    assert L.floria_hip_blob_estimate(None, None, None, C.c_uint32(1000), C.byref(state), C.byref(out)) == capi.FLORIA_E_INVALID
    assert b"null argument" in L.floria_hip_last_error() and not out
    L.floria_hip_estimate_result_free(None)


def test_the_model_on_a_hand_computed_pile():
    """five gapless records over [0, 10): the first column is sampled (count 0), its successor only counted; a sixth record whose bases end early"""
    recs = [(0, [(0, 10)], np.array([1] * 10))] * 3 + [(0, [(0, 10)], np.array([2] * 10)), (0, [(0, 4), (2, 2), (0, 4)], np.array([4] * 8)), (0, [(0, 10)], np.array([8] * 2))]
    got = model.estimate([recs], 1000)
    assert got["cols"] == [(0, 0, 6, 3)] and got["count"] == 10 and got["n_err"] == 1 and got["rec_hits"].tolist() == [1] * 6
    got = model.estimate([recs], 1000, count=995)                        # the column at 5: the deletion and the short record give nothing
    assert got["cols"] == [(0, 5, 4, 3), (0, 6, 5, 3)] and got["count"] == 1004 and got["rec_hits"].tolist() == [2, 2, 2, 2, 1, 0]
    assert model.result(got["cols"], model.lengths_of([recs], got["rec_hits"])) == (500, 2 / 3)
    assert model.result([], []) == (500, 0.01)
