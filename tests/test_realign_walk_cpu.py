"""`-m "not gpu"`: realign scored by a selectable member of the fixed-block walk family (floria-hip --realign block:STEP,RULE,TIE, floria_hip_realign_walk).
The definition is walk_score() of scripts/probes/block_walk.c.  Here: the Python models are that definition, the host twin (ingest.cpp: walk_affine_score) is the
model, the exact shortcut stays exact under every member, the command line's grammar, and the window set of the GPU test can tell the functions apart."""
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import realign_walk_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "floria-hip")


def ingest(floria_hip, prefix, tmp_path, extra=()):
    from tests.test_gpu_cli import parse_frag_dump
    dump = prefix + ".frags"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.03", "-l", "10000",
                        "--ingest-only", "--dump-frags", dump, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return parse_frag_dump(dump), r.stderr


def cells_of(pile):
    out = []
    for i in range(pile.n_reads):
        s, a, q = pile.read(i)
        out.append(list(zip(s.tolist(), a.tolist(), q.tolist())))
    return out


def test_python_models_are_the_c_definition(tmp_path):
    """Both Python models against scripts/probes/block_walk.c compiled here: the batch model (synth_bam.walk_affine_batch) on 2 400 windows at 10 % substitutions +
    5 indels, scores of both alleles and the calls, all 16 members; the line-by-line port (realign_walk_model.walk_score) on the first 40 of them, score and number
    of computed cells; and the exact DP of both sides."""
    L = M.c_definition(tmp_path)
    if L is None:
        pytest.skip("no C compiler (cc / gcc / clang) on this machine: the C definition cannot be compiled")
    Q, R0, R1, _ = M.windows(2400, 0.10, 5, 11)
    assert np.array_equal(M.exact_scores(Q, R0), M.c_batch(L, Q, R0, None)) and np.array_equal(M.exact_scores(Q, R1), M.c_batch(L, Q, R1, None))
    for member in M.MEMBERS:
        m0, cells = M.model_scores(Q, R0, member, want_cells=True)
        m1 = M.model_scores(Q, R1, member)
        c0, c1 = M.c_batch(L, Q, R0, member), M.c_batch(L, Q, R1, member)
        assert np.array_equal(m0, c0) and np.array_equal(m1, c1), member
        assert np.array_equal(m1 > m0, c1 > c0), member
        for x in range(40):
            want = M.c_walk(L, Q[x], R0[x], member)
            assert M.walk_score(Q[x], R0[x], 8, *member) == want, (member, x)
            assert (int(m0[x]), int(cells[x])) == want, (member, x)


def test_walk_never_scores_above_the_exact_dp():
    Q, R0, _, _ = M.windows(600, 0.2, 4, 3)
    e = M.exact_scores(Q, R0)
    for member in ((8, 0, 0), (4, 1, 1), (1, 0, 1)):
        assert (M.model_scores(Q, R0, member) <= e).all()


MEMBERS_ON_HOST = [(8, 0, 0), (4, 1, 1), (1, 0, 1)]


def test_host_twin_is_the_model(floria_hip, tmp_path):
    """floria-hip --ingest-only --realign block:... scores every undecided window on the host (walk_affine_score): its pileup is realign_dataset(d, walk=...).
    Reads with 50 % substitutions and an indel pair in every long read: noise at which, by the model alone, each tested member changes at least 5 calls of the exact
    DP's (asserted), so that the exact DP cannot pass for it.  --realign exact and no flag give today's pileup."""
    c = synth.make_config_contig(1, 0, keep_layout=True)
    prefix = str(tmp_path / "d")
    kw = dict(seed=4, sub_rate=0.5, edit_frac=1.0)
    exact = cells_of(synth_bam.write_dataset(prefix, [c], **kw)[c.name]["pileup"])
    got, _ = ingest(floria_hip, prefix, tmp_path)
    assert [g["cells"] for g in got[c.name]["reads"]] == exact
    got, _ = ingest(floria_hip, prefix, tmp_path, extra=("--realign", "exact"))
    assert [g["cells"] for g in got[c.name]["reads"]] == exact
    for member in MEMBERS_ON_HOST:
        want = cells_of(synth_bam.write_dataset(prefix, [c], walk=member, **kw)[c.name]["pileup"])
        n_diff = sum(1 for a, b in zip(want, exact) for x, y in zip(a, b) if x != y)
        print(f"{M.spec(member)}: {n_diff} calls differ from the exact DP's")
        assert len(want) == len(exact) and n_diff >= 5, (member, n_diff)
        got, _ = ingest(floria_hip, prefix, tmp_path, extra=("--realign", M.spec(member)))
        assert [g["cells"] for g in got[c.name]["reads"]] == want, member


def test_walk_options_of_the_dataset_helpers_default_to_today():
    c = synth.make_config_contig(4, 5, 0.3, keep_layout=True)
    d0 = synth_bam.contig_dataset(c, np.random.default_rng(2), sub_rate=0.1)
    d1 = synth_bam.contig_dataset(c, np.random.default_rng(2), sub_rate=0.1)
    assert synth_bam.realign_dataset(d0) == synth_bam.realign_dataset(d1, walk=None)
    assert [r[1] for r in d0["reads"]] == [r[1] for r in d1["reads"]]
    assert synth_bam.parse_walk((4, "sum", "down")) == (4, 1, 1) == synth_bam.parse_walk((4, 1, 1))
    for bad in ((3, 0, 0), (8, 2, 0), (8, 0, 2), (16, 0, 0)):
        with pytest.raises(ValueError):
            synth_bam.parse_walk(bad)


def shortcut_windows(n, seed):
    """substitution-only windows with h = 0 .. 4 mismatches outside the SNP column; the read's SNP base is allele 0, allele 1 or neither"""
    rng = np.random.default_rng(seed)
    R0 = M.BASES[rng.integers(0, 4, size=(n, 32))]
    R1 = R0.copy()
    R1[:, M.FL] = M.BASES[(np.searchsorted(M.BASES, R0[:, M.FL]) + rng.integers(1, 4, size=n)) % 4]
    Q = R0.copy()
    h = rng.integers(0, 5, size=n)
    kind = rng.integers(0, 3, size=n)
    for x in range(n):
        others = [b for b in M.BASES if b != R0[x, M.FL] and b != R1[x, M.FL]]
        Q[x, M.FL] = (R0[x, M.FL], R1[x, M.FL], others[int(rng.integers(0, 2))])[kind[x]]
        cols = rng.choice([k for k in range(32) if k != M.FL], size=int(h[x]), replace=False)
        Q[x, cols] = M.BASES[(np.searchsorted(M.BASES, Q[x, cols]) + rng.integers(1, 4, size=len(cols))) % 4]
    return Q, R0, R1, h, kind


def test_shortcut_is_exact_under_every_walk(floria_hip, tmp_path):
    """realign decides a window with h <= 2 mismatches outside the SNP column without a DP (ingest.cpp, "Exact shortcut"), which was proved for the exact DP.  It is
    kept under a walk.  A walk's score is never above the exact one, so the shortcut is right for a member iff the member still finds the ungapped alignment's score on
    such a window.  All 16 members, 3 000 windows, both sides of the bound: for h <= 2 (h <= 1 where the read's base is no allele) the walk's score of either allele is at
    least the main diagonal's (32 - 2h / 30 - 2h) and at most the exact DP's, its best score is the exact DP's, and its call is the shortcut's; for h = 3, 4 the host
    takes the DP anyway.  Then the host itself, shortcut and DP mixed, at 3 % and 12 %
    substitutions (0 .. 8 mismatches per window) under one member per step: its pileup is the model's, which scores every window."""
    Q, R0, R1, h, kind = shortcut_windows(3000, 5)
    e0, e1 = M.exact_scores(Q, R0), M.exact_scores(Q, R1)
    decided = np.where(kind == 2, h <= 1, h <= 2)
    assert decided.sum() > 1000 and (~decided).sum() > 1000
    shortcut_call = (kind == 1)                                        # the first allele equal to the read's base; none equal: allele 0
    ungapped = np.stack([32 - 2 * h - 2 * (kind != 0), 32 - 2 * h - 2 * (kind != 1)])     # the main diagonal's score under either allele
    assert np.array_equal(np.maximum(e0, e1)[decided], ungapped.max(axis=0)[decided])      # (the proof: the winner is ungapped; the loser at h = 2 may score 27 with gaps)
    for member in M.MEMBERS:
        w0, w1 = M.model_scores(Q, R0, member), M.model_scores(Q, R1, member)
        assert (w0 <= e0).all() and (w1 <= e1).all(), member
        assert (w0[decided] >= ungapped[0][decided]).all() and (w1[decided] >= ungapped[1][decided]).all(), member       # the walk holds the main diagonal
        assert np.array_equal(np.maximum(w0, w1)[decided], np.maximum(e0, e1)[decided]), member
        assert np.array_equal((w1 > w0)[decided], shortcut_call[decided]) and np.array_equal((e1 > e0)[decided], shortcut_call[decided]), member
        print(f"{M.spec(member)}: decided windows where a walk score differs from the exact DP's: {int(((w0 != e0) | (w1 != e1))[decided].sum())}")
    c = synth.make_config_contig(1, 0, 0.25, keep_layout=True)
    for sub_rate, members in ((0.03, [(8, 0, 0), (2, 1, 0)]), (0.12, [(4, 0, 1), (1, 1, 1)])):
        prefix = str(tmp_path / f"d{int(sub_rate * 100)}")
        for member in members:
            want = cells_of(synth_bam.write_dataset(prefix, [c], seed=4, sub_rate=sub_rate, walk=member)[c.name]["pileup"])
            got, _ = ingest(floria_hip, prefix, tmp_path, extra=("--realign", M.spec(member)))
            assert [g["cells"] for g in got[c.name]["reads"]] == want, (sub_rate, member)


def test_command_line_grammar(floria_hip, tmp_path):
    c = synth.make_config_contig(4, 5, 0.3, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=1)
    base = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.03", "-l", "10000", "--ingest-only"]
    for ok in ["exact"] + [M.spec(m) for m in M.MEMBERS]:
        r = subprocess.run(base + ["--realign", ok], capture_output=True, text=True)
        assert r.returncode == 0, (ok, r.stderr)
    for bad in ("block", "block:", "block:8", "block:8,max", "block:3,max,right", "block:16,max,right", "block:8,min,right", "block:8,max,left", "block:8,max,right,1",
                "block:08,max,right", "block:8, max,right", "Block:8,max,right", "banded", "", "block:8,MAX,right"):
        r = subprocess.run(base + ["--realign", bad], capture_output=True, text=True)
        assert r.returncode != 0, bad
        assert "exact | block:STEP,RULE,TIE" in r.stderr and "1 | 2 | 4 | 8" in r.stderr and "max | sum" in r.stderr and "right | down" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + ["--realign"], capture_output=True, text=True)
    assert r.returncode != 0
    for args in (["--no-realign", "--realign", "block:8,max,right"], ["--realign", "block:2,sum,down", "--no-realign"]):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode != 0 and "exclude each other" in r.stderr, r.stderr
    r = subprocess.run(base + ["--no-realign", "--realign", "exact"], capture_output=True, text=True)      # nothing to contradict
    assert r.returncode == 0, r.stderr
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--realign exact | block:STEP,RULE,TIE" in r.stderr + r.stdout


def test_library_refuses_unsupported_members_before_touching_a_device(hip_lib):
    """floria_hip_realign_walk validates its arguments first: a null context is FLORIA_E_INVALID, and the symbol exists (fails on a library without the feature)."""
    import ctypes as C
    from floria_amd import _capi as capi
    L = hip_lib.load()
    walk = capi.CRealignWalk(8, 3, 0, 0)
    buf = np.zeros(64, np.uint8)
    rc = L.floria_hip_realign_walk(None, capi.ptr(buf, C.c_uint8), capi.ptr(buf, C.c_uint8), capi.ptr(buf, C.c_uint8), capi.ptr(buf, C.c_uint8), C.c_uint64(1),
                                   C.byref(walk), capi.ptr(buf, C.c_uint8), None)
    assert rc == -1


def test_gpu_window_set_can_tell_the_functions_apart():
    """A condition on the GPU test's inputs, from the model alone: under every member at least 50 windows of the set have a score (of some allele) that differs from the
    exact DP's and at least 10 a different call, and each of step, rule and tie changes at least one score when it alone is changed.  A device that computed the exact
    DP, or another member, could not pass tests/test_gpu_realign_walk.py."""
    exact = M.gpu_set_scores(None)
    for member in M.MEMBERS:
        s = M.gpu_set_scores(member)
        n_score = int((s != exact).any(axis=0).sum()); n_call = int(((s[1] > s[0]) != (exact[1] > exact[0])).sum())
        print(f"{M.spec(member)}: {n_score} windows with a differing score, {n_call} with a differing call, of {s.shape[1]}")
        assert n_score >= 50 and n_call >= 10, (member, n_score, n_call)
    for step, rule, tie in M.MEMBERS:
        s = M.gpu_set_scores((step, rule, tie))
        for other in [(x, rule, tie) for x in (1, 2, 4, 8) if x != step] + [(step, 1 - rule, tie), (step, rule, 1 - tie)]:
            assert (M.gpu_set_scores(other) != s).any(), ((step, rule, tie), other)
