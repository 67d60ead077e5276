"""`-m gpu`: S2 with its epilogue on the device and the haplosets as a handle (csrc/haploset_kernel.h).  floria_hip_haplosets_download of
floria_hip_reassign_batch_resident against floria_hip_reassign_batch on the same inputs — n_groups, grp_off, grp_read, range — on the smallest shapes at which the
kernels can go wrong (tests/haploset_model.py: hand_cases) and on 300 random sparse short-read contigs (random_contig(seed), seeds 0 .. 299) in both arithmetics,
with and without a read order and under "s2_assign_only"; the four consumers by handle against their siblings on the downloaded groups, bit for bit; the handle's
residency; the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import haploset_model as hm

pytestmark = pytest.mark.gpu

N_RANDOM = 300


def same_groups(got, want, what=""):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.n_groups == w.n_groups, f"{what} contig {c}: {g.n_groups} groups instead of {w.n_groups}"
        assert np.array_equal(g.grp_off, w.grp_off), f"{what} contig {c}: grp_off"
        assert np.array_equal(g.grp_read, w.grp_read), f"{what} contig {c}: grp_read"
        assert np.array_equal(g.range, w.range), f"{what} contig {c}: range"


def both(ctx, contigs, gc, groups, ranges, eps, orders=None, what=""):
    want = ctx.reassign_batch(contigs, gc, groups, ranges, eps, orders)
    hs = ctx.reassign_batch_resident(contigs, gc, groups, ranges, eps, orders)
    same_groups(hs.download(), want, what)
    return hs, want


def flat(worlds):
    """[(spans, groups, ranges)] -> grp_contig, groups, ranges of one call"""
    gc, groups, ranges = [], [], []
    for c, (_, g, r) in enumerate(worlds):
        gc += [c] * len(g); groups += g; ranges += r
    return gc, groups, ranges


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    cases = hm.hand_cases()
    contigs = {name: gpu_ctx.upload(hm.reads_pileup(cases[name][0])) for name in cases}
    yield cases, contigs
    for c in contigs.values():
        c.free()


@pytest.fixture(scope="module")
def random_batch(gpu_ctx):
    worlds = [hm.random_contig(seed) for seed in range(N_RANDOM)]
    pileups = [hm.reads_pileup(w[0]) for w in worlds]
    assert max(p.n_reads for p in pileups) <= 200
    contigs = gpu_ctx.upload_batch(pileups)
    yield worlds, pileups, contigs
    for c in contigs:
        c.free()


# ---- (a) the smallest shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_wgs", [0, 1])
@pytest.mark.parametrize("name", sorted(hm.hand_cases()))
def test_hand_case(gpu_ctx, hand, name, chain_wgs):
    cases, contigs = hand
    spans, groups, ranges = cases[name]
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        hs, want = both(gpu_ctx, [contigs[name]], [0] * len(groups), groups, ranges, 0.03125, what=name)
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    f = [s[0] for s in spans]; l = [s[1] for s in spans]
    parts, rng = hm.epilogue(f, l, groups, ranges)                    # disjoint groups: the model's input is exact
    got = hs.download()[0]
    assert [list(map(int, got.group(g))) for g in range(got.n_groups)] == parts and [tuple(map(int, r)) for r in got.range] == rng
    hs.free()


@pytest.mark.parametrize("chain_wgs", [0, 1])
def test_several_contigs_in_one_call(gpu_ctx, hand, chain_wgs):
    """every hand case as a contig of one call, plus a contig without groups and one whose groups hold no read"""
    cases, contigs = hand
    names = sorted(cases)
    worlds = [cases[n] for n in names]
    worlds.insert(3, (cases["one_gap"][0], [], []))                                   # no group at all
    worlds.insert(7, (cases["two_gaps"][0], [[], [], []], [(5, 9), (1, 3), (5, 9)]))     # groups, none with a read: they stay, sorted
    hc = [contigs[n] for n in names]
    hc.insert(3, contigs["one_gap"]); hc.insert(7, contigs["two_gaps"])
    gc, groups, ranges = flat(worlds)
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        hs, want = both(gpu_ctx, hc, gc, groups, ranges, 0.03125, what="all hand cases")
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    assert want[3].n_groups == 0 and want[7].n_groups == 3 and len(want[7].grp_read) == 0 and [tuple(r) for r in want[7].range] == [(1, 3), (5, 9), (5, 9)]
    t = gpu_ctx.timing()
    assert t["select_ms"] > 0 and t["d2h_ms"] > 0
    hs.free()


def test_no_group_and_no_contig(gpu_ctx, hand):
    cases, contigs = hand
    hs, want = both(gpu_ctx, [contigs["one_gap"]], [], [], [], 0.03125)
    assert want[0].n_groups == 0
    assert gpu_ctx.haploset_stats([contigs["one_gap"]], haplosets=hs).shape == (0, 4)
    hs.free()
    hs = gpu_ctx.reassign_batch_resident([], [], [], [], 0.03125)
    assert hs.download() == []
    hs.free()


# ---- (b) random sparse short-read contigs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("arith,eps", [(0, 0.03125), (0, 0.04), (1, 0.03125), (1, 0.04)])
def test_random_contigs(gpu_ctx, random_batch, arith, eps, ordered):
    worlds, pileups, contigs = random_batch
    gc, groups, ranges = flat(worlds)
    orders = None
    if ordered:
        rng = np.random.default_rng(41)
        orders = [rng.permutation(p.n_reads).astype(np.uint32) for p in pileups]
    gpu_ctx.set_option("arith", arith)
    try:
        hs, want = both(gpu_ctx, contigs, gc, groups, ranges, eps, orders, what=f"arith {arith} eps {eps}")
    finally:
        gpu_ctx.set_option("arith", 0)
    split = sum(w.n_groups > len(world[1]) for w, world in zip(want, worlds))
    assert split * 5 > N_RANDOM, f"only {split} of {N_RANDOM} contigs split"
    hs.free()


def test_random_contigs_assign_only_and_one_workgroup(gpu_ctx, random_batch):
    worlds, pileups, contigs = random_batch
    gc, groups, ranges = flat(worlds)
    gpu_ctx.set_option("s2_assign_only", 1)
    try:
        hs, want = both(gpu_ctx, contigs, gc, groups, ranges, 0.04, what="assign only")
    finally:
        gpu_ctx.set_option("s2_assign_only", 0)
    assert all(w.n_groups == len(world[1]) and [tuple(r) for r in w.range] == [tuple(r) for r in world[2]] for w, world in zip(want, worlds))
    hs.free()
    gpu_ctx.set_option("chain_wgs", 1)                                  # every wavefront meets many groups and contigs
    try:
        hs, _ = both(gpu_ctx, contigs[:60], *flat(worlds[:60]), 0.04, what="one workgroup")
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    hs.free()


# ---- (c) the consumers by handle ---------------------------------------------------------------------------------------------------------------------------------
def listed(want):
    gc, groups, ranges = [], [], []
    for c, w in enumerate(want):
        for g in range(w.n_groups):
            gc.append(c); groups.append(w.group(g)); ranges.append(tuple(map(int, w.range[g])))
    return gc, groups, ranges


def snp_positions(worlds):
    """a base position for every SNP a range or a read of the contig names"""
    return [np.arange(1, max([hi for _, hi in w[2]] + [l for _, l in w[0]]) + 2, dtype=np.uint64) * 137 for w in worlds]


def test_stats_hapq_alleles_by_handle(gpu_ctx, random_batch):
    worlds, pileups, contigs = random_batch
    n = 80
    hs, want = both(gpu_ctx, contigs[:n], *flat(worlds[:n]), 0.04)
    gc, groups, ranges = listed(want)
    assert any(len(g) == 0 for g in groups) and len(groups) == hs.n_groups
    a = gpu_ctx.haploset_stats(contigs[:n], haplosets=hs)
    b = gpu_ctx.haploset_stats(contigs[:n], gc, groups, ranges)
    assert np.isnan(b).any() and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    pos = snp_positions(worlds[:n])
    ha = gpu_ctx.hapq_batch(contigs[:n], snp_positions=pos, block_length=5000, haplosets=hs)
    hb = gpu_ctx.hapq_batch(contigs[:n], gc, groups, ranges, pos, 5000)
    assert np.array_equal(ha[0], hb[0]) and (hb[0] > 0).any()
    assert np.array_equal(ha[1].view(np.uint64), hb[1].view(np.uint64)) and np.array_equal(ha[2].view(np.uint64), hb[2].view(np.uint64))
    ha2 = gpu_ctx.hapq_batch(contigs[:n], snp_positions=pos, block_length=5000, haplosets=hs)      # the handle's cached spans
    assert np.array_equal(ha[0], ha2[0]) and np.array_equal(ha[1].view(np.uint64), ha2[1].view(np.uint64))
    pa, ca = gpu_ctx.haploset_alleles(contigs[:n], haplosets=hs)
    pb, cb = gpu_ctx.haploset_alleles(contigs[:n], gc, groups, ranges)
    assert np.array_equal(pa, pb) and np.array_equal(ca, cb) and cb.any()
    hs.free()


def test_read_spans_by_handle(gpu_ctx):
    from tests.test_gpu_assemble import free_all, resident
    from tests.test_gpu_spans import assemble_sp, span_world
    recs, tables, walked, plan, mate, counts = span_world()
    s = resident(gpu_ctx, recs, tables)
    got = assemble_sp(gpu_ctx, s, plan, mate)
    pileups = plan["pileups"]
    gc, groups, ranges = [], [], []
    for c, p in enumerate(pileups):
        lo, hi = int(p.first.min()), int(p.last.max())
        ids = np.arange(p.n_reads)
        gc += [c, c, c]; groups += [ids[::2], ids[1::2], ids[:0]]; ranges += [(lo, hi), (lo + 1, max(lo + 1, hi - 1)), (lo, lo + 3)]
    hs, want = both(gpu_ctx, got, gc, groups, ranges, 0.04)
    lgc, lgroups, lranges = listed(want)
    la, ra = gpu_ctx.read_spans(got, haplosets=hs)
    lb, rb = gpu_ctx.read_spans(got, lgc, lgroups, lranges)
    assert len(la) == hs.n_entries > 0 and np.array_equal(la, lb) and np.array_equal(ra, rb)
    hs.free()
    free_all(got); s.free()


# ---- (d) residency -----------------------------------------------------------------------------------------------------------------------------------------------
def test_handle_survives_later_calls(gpu_ctx, hip_lib, random_batch):
    worlds, pileups, contigs = random_batch
    hs, want = both(gpu_ctx, contigs[:40], *flat(worlds[:40]), 0.04)
    st = gpu_ctx.haploset_stats(contigs[:40], haplosets=hs)
    # a later S1 batch, another S2 call by arrays and another resident one (on other contigs) ...
    p = pileups[50]
    gpu_ctx.phase_blocks_batch(contigs[50:52], [0, 1], [1, 1], [int(p.last.max()), int(pileups[51].last.max())], hip_lib.make_params(0.04, max_ploidy=2))
    other, _ = both(gpu_ctx, contigs[100:160], *flat(worlds[100:160]), 0.03125)
    # ... and the first handle answers the same: a fresh download, and a consumer
    hs._groups = None
    same_groups(hs.download(), want, "after later calls")
    assert np.array_equal(gpu_ctx.haploset_stats(contigs[:40], haplosets=hs).view(np.uint64), st.view(np.uint64))
    other.free()
    hs._groups = None
    same_groups(hs.download(), want, "after freeing another handle")
    hs.free()


# ---- (e) refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, hip_lib, random_batch):
    worlds, pileups, contigs = random_batch
    cs = contigs[:5]
    hs, want = both(gpu_ctx, cs, *flat(worlds[:5]), 0.04)
    pos = snp_positions(worlds[:5])
    calls = {
        "haploset_stats_resident": lambda ctx, c: ctx.haploset_stats(c, haplosets=hs),
        "hapq_batch_resident": lambda ctx, c: ctx.hapq_batch(c, snp_positions=pos[:len(c)], block_length=5000, haplosets=hs),
        "haploset_alleles_resident": lambda ctx, c: ctx.haploset_alleles(c, haplosets=hs),
        "read_spans_resident": lambda ctx, c: ctx.read_spans(c, haplosets=hs),
    }

    def refused(f, *args, msg):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            f(*args)
        assert ei.value.code == -1 and msg in str(ei.value), str(ei.value)

    other = hip_lib.FloriaHip(0)
    try:
        for who, f in calls.items():
            refused(f, other, cs, msg=who + ": the haplosets belong to another context")
            refused(f, gpu_ctx, cs[:4], msg=who + ": 4 contigs given, the haplosets were made from 5")
            refused(f, gpu_ctx, cs[:3] + [cs[4], cs[3]], msg=who + ": contig 3 is not the one the haplosets were made from")
            refused(f, gpu_ctx, cs[:4] + [contigs[9]], msg=who + ": contig 4 is not the one the haplosets were made from")
    finally:
        other.close()
    refused(calls["read_spans_resident"], gpu_ctx, cs, msg="the contig carries no seq_pos")          # the sibling's message
    # null arguments, by the C entry points themselves
    L = hip_lib.load()
    arr = (C.c_void_p * 5)(*[c._h for c in cs])
    out = np.zeros((hs.n_groups + 1, 4), np.float64)
    cnt = np.zeros(16, np.uint32)
    nulls = [lambda: L.floria_hip_haploset_stats_resident(gpu_ctx._h, arr, 5, None, out.ctypes.data_as(C.POINTER(C.c_double))),
             lambda: L.floria_hip_haploset_stats_resident(None, arr, 5, hs._h, out.ctypes.data_as(C.POINTER(C.c_double))),
             lambda: L.floria_hip_haploset_stats_resident(gpu_ctx._h, None, 5, hs._h, out.ctypes.data_as(C.POINTER(C.c_double))),
             lambda: L.floria_hip_haploset_stats_resident(gpu_ctx._h, arr, 5, hs._h, None),
             lambda: L.floria_hip_haploset_alleles_resident(gpu_ctx._h, arr, 5, hs._h, None, cnt.ctypes.data_as(C.POINTER(C.c_uint32))),
             lambda: L.floria_hip_read_spans_resident(gpu_ctx._h, arr, 5, None, None, None),
             lambda: L.floria_hip_hapq_batch_resident(gpu_ctx._h, arr, 5, hs._h, None, None, 5000, None, None, None),
             lambda: L.floria_hip_haplosets_download(None, None),
             lambda: L.floria_hip_haplosets_download(hs._h, None)]
    for f in nulls:
        assert f() == -1 and b"null argument" in L.floria_hip_last_error()
    holey = (C.c_void_p * 5)(*[c._h for c in cs]); holey[2] = None
    assert L.floria_hip_haploset_stats_resident(gpu_ctx._h, holey, 5, hs._h, out.ctypes.data_as(C.POINTER(C.c_double))) == -1
    # the S2 call itself refuses what floria_hip_reassign_batch refuses, with its messages
    gc, groups, ranges = flat(worlds[:5])
    for bad, msg in (((cs, gc, [np.array([10 ** 6])] + groups[1:], ranges, 0.04), "group read id out of range"),
                     ((cs, [7] + gc[1:], groups, ranges, 0.04), "grp_contig out of range"),
                     ((cs, gc, groups, ranges, 0.04, [np.zeros(2, np.uint32)] * 5), "read_order")):
        errs = []
        for f in (gpu_ctx.reassign_batch, gpu_ctx.reassign_batch_resident):
            with pytest.raises(hip_lib.FloriaHipError) as ei:
                f(*bad)
            errs.append((ei.value.code, str(ei.value)))
        assert errs[0] == errs[1] and msg in errs[0][1], errs
    # and the handle still answers
    hs._groups = None
    same_groups(hs.download(), want, "after the refusals")
    hs.free()
