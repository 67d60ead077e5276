"""`-m gpu`: floria_hip_reassign_haplosets_resident — S2 whose input groups are a floria_hip_haplosets handle, its per-read tables built on the device
(csrc/haploset_kernel.h: hp_*).  floria_hip_haplosets_download(out) against floria_hip_reassign_batch_resident on floria_hip_haplosets_download(in), list for list:
with `in` an earlier S2 output (the hand cases of tests/haploset_model.py, taken under "s2_assign_only" so that the handle holds exactly the case's groups) and with
`in` from floria_hip_join_paths (reads with a choice between two and between three groups, an empty group, a contig without groups, one without a read that has a
choice, groups of 64 / 65 / 129 reads; the 300 random sparse contigs at both epsilons in both arithmetics, under "s2_assign_only" and "reassign_path" 1 and 2); `in`
unchanged afterwards; the refusals."""
import numpy as np
import pytest

from tests import haploset_model as hm
from tests import join_cases as jc
from tests import join_model as jm
from tests.test_gpu_haplosets import flat, same_groups

pytestmark = pytest.mark.gpu


def check(ctx, contigs, hin, eps, what=""):
    """out = S2(handle) against S2(download(handle)); `hin` must come through unchanged -> (out, want)"""
    before = hin.download()
    gc, groups, ranges = jc.listed(before)
    out = ctx.reassign_haplosets_resident(contigs, hin, eps)
    want = ctx.reassign_batch_resident(contigs, gc, groups, ranges, eps)
    same_groups(out.download(), want.download(), what)
    hin._groups = None
    same_groups(hin.download(), before, what + ": the input handle")
    want.free()
    return out


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    cases = hm.hand_cases()
    names = sorted(cases)
    contigs = gpu_ctx.upload_batch([hm.reads_pileup(cases[n][0]) for n in names])
    yield cases, names, contigs
    for c in contigs:
        c.free()


@pytest.fixture(scope="module")
def sized(gpu_ctx, hip_lib):
    w = jc.sized_world()
    w["contigs"] = gpu_ctx.upload_batch(w["pileups"])
    prm = hip_lib.make_params(0.04, max_ploidy=1)          # ploidy 1: node (b, 0) is the whole list of block b
    w["phase"] = lambda: gpu_ctx.phase_blocks_batch(w["contigs"], w["bc"], w["bs"], w["be"], prm)
    yield w
    for c in w["contigs"]:
        c.free()


@pytest.fixture(scope="module")
def rand(gpu_ctx, hip_lib):
    w = jc.random_world()
    w["contigs"] = gpu_ctx.upload_batch(w["pileups"])
    prm = hip_lib.make_params(0.04, max_ploidy=2)
    w["phase"] = lambda: gpu_ctx.phase_blocks_batch(w["contigs"], w["bc"], w["bs"], w["be"], prm)
    yield w
    for c in w["contigs"]:
        c.free()


# ---- `in` is an earlier S2 output ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_wgs", [0, 1])
def test_hand_cases_from_an_s2_output(gpu_ctx, hand, chain_wgs):
    cases, names, contigs = hand
    worlds = [cases[n] for n in names]
    gc, groups, ranges = flat(worlds)
    gpu_ctx.set_option("s2_assign_only", 1)                # the groups as given: disjoint, so the re-insertion leaves them as they are
    try:
        hin = gpu_ctx.reassign_batch_resident(contigs, gc, groups, ranges, 0.03125)
    finally:
        gpu_ctx.set_option("s2_assign_only", 0)
    got = jc.listed(hin.download())
    assert got[0] == gc and all(np.array_equal(a, np.asarray(b, np.uint32)) for a, b in zip(got[1], groups)) and got[2] == [tuple(r) for r in ranges]
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        out = check(gpu_ctx, contigs, hin, 0.03125, "hand cases")
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    for c, n in enumerate(names):                          # ... and the model's splits, case by case
        spans, g, r = cases[n]
        parts, rng = hm.epilogue([s[0] for s in spans], [s[1] for s in spans], g, r)
        d = out.download()[c]
        assert [list(map(int, d.group(i))) for i in range(d.n_groups)] == parts and [tuple(map(int, x)) for x in d.range] == rng, n
    again = check(gpu_ctx, contigs, out, 0.03125, "an S2 output of an S2 output")
    again.free(); out.free(); hin.free()


def test_no_group_and_no_contig(gpu_ctx, hand):
    cases, names, contigs = hand
    hin = gpu_ctx.reassign_batch_resident(contigs[:2], [], [], [], 0.04)
    out = check(gpu_ctx, contigs[:2], hin, 0.04)
    assert [g.n_groups for g in out.download()] == [0, 0]
    out.free(); hin.free()
    hin = gpu_ctx.reassign_batch_resident([], [], [], [], 0.04)
    out = gpu_ctx.reassign_haplosets_resident([], hin, 0.04)
    assert out.download() == []
    out.free(); hin.free()


# ---- `in` comes from floria_hip_join_paths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_wgs", [0, 1])
def test_choices_sizes_and_empty_groups(gpu_ctx, sized, chain_wgs):
    w = sized
    res = w["phase"]()
    assert (res.best_ploidy[np.diff(res.read_off.astype(np.int64)) > 0] == 1).all()
    s = w["sized"]
    sb = w["small_blocks"]
    # contig 0: the five overlapping blocks as a group each (a read of two or three consecutive blocks has that many candidates), the lists of 64 / 65 / 129 reads, an
    # empty group; contig 1: one group (no read has a choice); contig 2: the two ends; contig 3: no group; contig 4: three overlapping blocks and their union
    pc = [0] * 9 + [1] + [2, 2] + [4] * 4
    nodes = [[(b, 0)] for b in range(5)] + [[(s[64], 0)], [(s[65], 0)], [], [(s[129], 0)]] + [[(w["gap_blocks"], 0), (w["gap_blocks"] + 2, 0)]] + \
            [[(w["big_blocks"], 0)], [(w["big_blocks"] + 1, 0)]] + [[(sb, 0)], [(sb + 1, 0)], [(sb + 2, 0)], [(sb, 0), (sb + 1, 0), (sb + 2, 0)]]
    ranges = [(int(w["bs"][n[0][0]]), int(w["be"][n[-1][0]])) if n else (3, 4) for n in nodes]
    want = jc.model_groups(res, nodes)
    assert [len(want[i]) for i in (5, 6, 7, 8)] == [64, 65, 0, 129]
    c0 = jm.candidates(want[:9], w["pileups"][0].n_reads)
    assert (c0 == 2).any() and (c0 == 3).any(), np.bincount(c0)
    assert jm.candidates(want[9:10], w["pileups"][1].n_reads).max() == 1
    hin = gpu_ctx.join_paths(res, w["contigs"], pc, nodes, ranges)
    jc.same_as_model(hin.download(), pc, want, ranges, 5, "join")
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        out = check(gpu_ctx, w["contigs"], hin, 0.04, "sized world")
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    assert out.download()[3].n_groups == 0 and out.n_entries > 0
    out.free(); hin.free()


def joined_random(gpu_ctx, w, seed):
    res = w["phase"]()
    pc, nodes, ranges = jc.random_paths(res, w["bc"], jc.N_RANDOM, seed=seed)
    hin = gpu_ctx.join_paths(res, w["contigs"], pc, nodes, ranges)
    groups = jc.model_groups(res, nodes)
    cand = [jm.candidates(g, p.n_reads) for (g, _), p in zip(jc.per_contig(pc, groups, ranges, jc.N_RANDOM), w["pileups"])]
    assert sum(int((c == 2).sum()) for c in cand) > 100 and sum(int((c >= 3).sum()) for c in cand) > 20, "too few reads with a choice"
    return hin


@pytest.mark.parametrize("arith,eps", [(0, 0.03125), (0, 0.04), (1, 0.03125), (1, 0.04)])
def test_random_contigs_from_a_join(gpu_ctx, rand, arith, eps):
    hin = joined_random(gpu_ctx, rand, seed=3)
    gpu_ctx.set_option("arith", arith)
    try:
        out = check(gpu_ctx, rand["contigs"], hin, eps, f"arith {arith} eps {eps}")
    finally:
        gpu_ctx.set_option("arith", 0)
    out.free(); hin.free()


@pytest.mark.parametrize("key,value", [("s2_assign_only", 1), ("reassign_path", 1), ("reassign_path", 2), ("chain_wgs", 1)])
def test_random_contigs_under_options(gpu_ctx, rand, key, value):
    hin = joined_random(gpu_ctx, rand, seed=4)
    gpu_ctx.set_option(key, value)
    try:
        out = check(gpu_ctx, rand["contigs"], hin, 0.04, f"{key} = {value}")
        second = check(gpu_ctx, rand["contigs"], out, 0.03125, f"{key} = {value}, from the S2 output")
    finally:
        gpu_ctx.set_option(key, 0)
    second.free(); out.free(); hin.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, hip_lib, hand):
    cases, names, contigs = hand
    cs = contigs[:5]
    worlds = [cases[n] for n in names[:5]]
    hin = gpu_ctx.reassign_batch_resident(cs, *flat(worlds), 0.04)
    before = hin.download()

    def refused(ctx, c, h, msg):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            ctx.reassign_haplosets_resident(c, h, 0.04)
        assert ei.value.code == -1 and msg in str(ei.value), str(ei.value)

    who = "reassign_haplosets_resident"
    other = hip_lib.FloriaHip(0)
    try:
        refused(other, cs, hin, who + ": the haplosets belong to another context")
    finally:
        other.close()
    refused(gpu_ctx, cs[:4], hin, who + ": 4 contigs given, the haplosets were made from 5")
    refused(gpu_ctx, cs[:3] + [cs[4], cs[3]], hin, who + ": contig 3 is not the one the haplosets were made from")
    refused(gpu_ctx, cs[:4] + [contigs[9]], hin, who + ": contig 4 is not the one the haplosets were made from")
    refused(gpu_ctx, cs, None, "null argument")
    refused(gpu_ctx, None, hin, "null argument")
    L = hip_lib.load()
    assert L.floria_hip_reassign_haplosets_resident(None, None, 0, hin._h, 0.04, None) == -1 and b"null argument" in L.floria_hip_last_error()
    hin._groups = None
    same_groups(hin.download(), before, "after the refusals")
    hin.free()
