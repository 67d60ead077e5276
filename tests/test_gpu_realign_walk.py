"""`-m gpu`: floria_hip_realign_walk (realign_walk_kernel.h) against the model of the fixed-block walk family (tests/realign_walk_model.py, pinned to the C
definition by tests/test_realign_walk_cpu.py), and floria-hip --realign block:... end to end.  Nothing here asks the device for anything it may refuse at run time:
the invalid members are refused by the host part of the entry point before any launch."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import realign_walk_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "floria-hip")


def two_alleles(R0, R1):
    al = np.zeros((len(R0), 4), np.uint8)
    al[:, 0] = R0[:, M.FL]; al[:, 1] = R1[:, M.FL]
    return al, np.full(len(R0), 2, np.uint8)


@pytest.mark.parametrize("member", M.MEMBERS, ids=M.spec)
def test_device_is_the_model_and_differs_from_the_exact_kernel_where_the_model_does(gpu_ctx, member):
    """13 999 noisy, indel-rich windows (a count that fills neither the last workgroup nor the last wavefront), two alleles each: best score and first-best call of the
    device == the model's under this member; and the windows on which the device's walk score differs from the device's exact score (floria_hip_realign, same context)
    are exactly those on which the model's walk score differs from the model's exact score - at least 50 of them (test_gpu_window_set_can_tell_the_functions_apart), so
    an entry point wired to the exact kernel, or to another member, fails here."""
    Q, R0, R1 = M.gpu_set()
    al, na = two_alleles(R0, R1)
    want_call, want_score = M.first_best(M.gpu_set_scores(member))
    exact_call, exact_score = M.first_best(M.gpu_set_scores(None))
    call, score = gpu_ctx.realign_walk(Q, R0, al, na, *member, want_scores=True)
    n_bad = int((score != want_score).sum())
    print(f"{M.spec(member)}: {n_bad} of {len(Q)} scores differ from the model's, {int((call != want_call).sum())} calls")
    assert np.array_equal(score, want_score), f"{n_bad} scores differ, first at {np.nonzero(score != want_score)[0][:8]}"
    assert np.array_equal(call, want_call)
    assert np.array_equal(gpu_ctx.realign_walk(Q, R0, al, na, *member), want_call)                 # without the score output
    dev_exact_call, dev_exact_score = gpu_ctx.realign(Q, R0, al, na, want_scores=True)
    assert np.array_equal(dev_exact_score, exact_score) and np.array_equal(dev_exact_call, exact_call)
    assert np.array_equal(score != dev_exact_score, want_score != exact_score) and int((score != dev_exact_score).sum()) >= 50
    assert np.array_equal(call != dev_exact_call, want_call != exact_call) and int((call != dev_exact_call).sum()) >= 10


@pytest.mark.parametrize("n", [0, 1, 3, 17, 2999])
def test_one_to_four_alleles_ties_and_odd_counts(gpu_ctx, n):
    """1-4 candidate alleles per window, a quarter of them repeating their predecessor (equal scores: the FIRST best allele wins, strict >), for window counts that are
    0, below one wavefront's four windows, and no multiple of a workgroup's sixteen; every member."""
    Q, R, al, na = M.multi_allele_set(max(n, 1), 21)
    Q, R, al, na = Q[:n], R[:n], al[:n], na[:n]
    if n >= 17:
        assert set(na.tolist()) == {1, 2, 3, 4}
    for member in M.MEMBERS:
        call, score = gpu_ctx.realign_walk(Q, R, al, na, *member, want_scores=True)
        assert call.shape == (n,) and score.shape == (n,)
        if n == 0:
            continue
        s = M.multi_allele_scores(Q, R, al, na, member)
        want_call, want_score = M.first_best(s)
        assert np.array_equal(score, want_score) and np.array_equal(call, want_call), member
        if n == 2999:
            tied = (s == want_score).sum(axis=0) > 1
            assert tied.sum() > 100 and (want_call[tied] == np.argmax(s[:, tied] == want_score[tied], axis=0)).all()


@pytest.mark.parametrize("member", [(8, 0, 0), (2, 0, 1), (1, 1, 1)], ids=M.spec)
def test_more_windows_than_one_pass_of_the_grid(gpu_ctx, member):
    """The launcher caps the grid at 32 workgroups per CU; beyond 16 windows x that many workgroups a 16-lane group takes several windows in turn.  2 999 windows with 1-4
    alleles repeated 139 times (416 861 windows: more than a capped grid of any device with up to 800 CUs covers in one pass, and no multiple of 16): every copy scores as
    the model's one."""
    Q, R, al, na = M.multi_allele_set(2999, 21)
    want_call, want_score = M.first_best(M.multi_allele_scores(Q, R, al, na, member))
    k = 139
    call, score = gpu_ctx.realign_walk(np.tile(Q, (k, 1)), np.tile(R, (k, 1)), np.tile(al, (k, 1)), np.tile(na, k), *member, want_scores=True)
    assert np.array_equal(score, np.tile(want_score, k)) and np.array_equal(call, np.tile(want_call, k))


def test_invalid_members_are_refused_and_the_context_stays_usable(gpu_ctx, hip_lib):
    Q, R0, R1, _ = M.windows(64, 0.1, 2, 5)
    al, na = two_alleles(R0, R1)
    before = gpu_ctx.realign(Q, R0, al, na, want_scores=True)
    for block, step, rule, tie in ((16, 8, 0, 0), (4, 4, 0, 0), (0, 8, 0, 0), (8, 0, 0, 0), (8, 3, 0, 0), (8, 16, 0, 0), (8, 8, 2, 0), (8, 8, 0, 2), (8, 8, 0, 0xffffffff)):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.realign_walk(Q, R0, al, na, step, rule, tie, block=block)
        assert ei.value.code == -1, (block, step, rule, tie)
        msg = str(ei.value)
        assert "block must be 8" in msg and "1, 2, 4 or 8" in msg and "max" in msg and "sum" in msg and "right" in msg and "down" in msg, msg
    bad_na = na.copy(); bad_na[5] = 5
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        gpu_ctx.realign_walk(Q, R0, al, bad_na, 8, 0, 0)
    assert ei.value.code == -1
    after = gpu_ctx.realign(Q, R0, al, na, want_scores=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    call, score = gpu_ctx.realign_walk(Q, R0, al, na, 8, "max", "right", want_scores=True)
    want_call, want_score = M.first_best(np.stack([M.model_scores(Q, R0, (8, 0, 0)), M.model_scores(Q, R1, (8, 0, 0))]))
    assert np.array_equal(call, want_call) and np.array_equal(score, want_score)


def run_cli(floria_hip, prefix, cwd, dump, extra=()):
    """-> stderr of a run that writes ./out under `cwd` (the vartig and haploset headers hold the output directory as given: the same relative name in every run)"""
    os.makedirs(cwd)
    cmd = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", "out", "-e", "0.03125", "-l", "10000", "--dump-frags", dump, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r.stderr


def test_cli_end_to_end_on_noisy_long_reads(floria_hip, tmp_path):
    """floria-hip --realign block:8,max,right on long reads with 50 % substitutions and indels: the windows the shortcut cannot decide are scored by
    floria_hip_realign_walk, the pileup is realign_dataset(d, walk=...) and differs from the exact DP's pileup (so the exact kernel cannot pass), the log line and
    cmd.log name the scoring.  The same data with no flag and with --realign exact: today's pileup, and the same files byte for byte."""
    from tests.test_gpu_cli import parse_frag_dump
    from tests.test_realign_walk_cpu import cells_of
    member = (8, 0, 0)
    c = synth.make_config_contig(1, 0, keep_layout=True)
    prefix = str(tmp_path / "d")
    kw = dict(seed=4, sub_rate=0.5, edit_frac=1.0)
    exact = cells_of(synth_bam.write_dataset(prefix, [c], **kw)[c.name]["pileup"])
    want = cells_of(synth_bam.write_dataset(prefix, [c], walk=member, **kw)[c.name]["pileup"])
    assert sum(1 for a, b in zip(want, exact) for x, y in zip(a, b) if x != y) >= 5
    outs = {}
    for tag, extra in (("walk", ("--realign", M.spec(member))), ("default", ()), ("exact", ("--realign", "exact"))):
        out, dump = str(tmp_path / tag / "out"), str(tmp_path / f"frags_{tag}.txt")
        log = run_cli(floria_hip, prefix, str(tmp_path / tag), dump, extra)
        line = [ln for ln in log.splitlines() if ln.startswith("Realignment:")]
        assert len(line) == 1 and int(re.search(r"Realignment: (\d+) calls scored on the device", line[0]).group(1)) > 1000, log
        note = open(os.path.join(out, "cmd.log")).read()
        if tag == "walk":
            assert "fixed-block walk block:8,max,right" in line[0] and "fixed-block walk block:8,max,right" in note
        else:
            assert "exact affine-gap DP" in line[0] and "fixed-block walk" not in note
        outs[tag] = (out, [g["cells"] for g in parse_frag_dump(dump)[c.name]["reads"]])
    assert outs["walk"][1] == want
    assert outs["default"][1] == exact and outs["exact"][1] == exact
    # no flag == --realign exact, file by file (cmd.log records the command line itself and is the one file that must differ)
    cmp = filecmp.dircmp(outs["default"][0], outs["exact"][0])
    stack, n_files = [cmp], 0
    while stack:
        d = stack.pop()
        assert not d.left_only and not d.right_only, (d.left_only, d.right_only)
        for f in d.common_files:
            if f == "cmd.log" and d is cmp:
                continue
            assert filecmp.cmp(os.path.join(d.left, f), os.path.join(d.right, f), shallow=False), f
            n_files += 1
        stack.extend(d.subdirs.values())
    assert n_files >= 3
