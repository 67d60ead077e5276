"""`-m gpu`: floria_hip_join_paths (csrc/path_kernel.h) — hap-graph paths joined into haplosets on the S1 batch that is still resident.  The download of the joined
handle against tests/join_model.py on paths built FROM the S1 result (tests/join_cases.py), each phenomenon asserted present: a read two nodes of a path share, a
read in two groups, a one-node path, a path without nodes, a path that skips an empty block, lists of 64 / 65 / 129 entries, a window of more than 64 x 64 ids, five
contigs of which one has no path; every case again under "chain_wgs" = 1; 300 random contigs with random node lists; the same call under "s1_no_lists" = 1 and
before / after floria_hip_hap_graph; floria_hip_haploset_stats_resident on a joined handle; every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import join_cases as jc
from tests import join_model as jm

pytestmark = pytest.mark.gpu

EPS = 0.04


@pytest.fixture(scope="module")
def sized(gpu_ctx, hip_lib):
    w = jc.sized_world()
    contigs = gpu_ctx.upload_batch(w["pileups"])
    prm = hip_lib.make_params(EPS, max_ploidy=3)
    w["contigs"] = contigs
    w["phase"] = lambda: gpu_ctx.phase_blocks_batch(contigs, w["bc"], w["bs"], w["be"], prm)
    w["res"] = w["phase"]()
    w["cases"] = sized_cases(w)
    yield w
    for c in contigs:
        c.free()


@pytest.fixture(scope="module")
def rand(gpu_ctx, hip_lib):
    w = jc.random_world()
    contigs = gpu_ctx.upload_batch(w["pileups"])
    prm = hip_lib.make_params(EPS, max_ploidy=2)
    w["contigs"] = contigs
    w["phase"] = lambda: gpu_ctx.phase_blocks_batch(contigs, w["bc"], w["bs"], w["be"], prm)
    w["res"] = w["phase"]()
    yield w
    for c in contigs:
        c.free()


def sized_cases(w):
    """name -> (path_contig, nodes, ranges), built from the S1 result; asserts that every phenomenon is there."""
    res, bc = w["res"], w["bc"]
    ro, rid, part = res.read_off, res.read_id, res.part
    cnt = np.diff(ro.astype(np.int64))
    bp = res.best_ploidy
    cases = {}
    # two consecutive blocks' nodes that share a read, in one path
    shared = None
    for b in range(w["n_main_regular"] - 1):
        for k1 in range(int(bp[b])):
            for k2 in range(int(bp[b + 1])):
                if shared is None and len(np.intersect1d(jm.node_reads(ro, rid, part, b, k1), jm.node_reads(ro, rid, part, b + 1, k2))):
                    shared = ((b, k1), (b + 1, k2))
    assert shared is not None, "no two consecutive blocks share a read"
    a, b = shared
    both = np.concatenate([jm.node_reads(ro, rid, part, *a), jm.node_reads(ro, rid, part, *b)])
    assert len(np.unique(both)) < len(both)
    cases["dedupe"] = ([0], [[a, b]], [(1, 300)])
    # the same read's two nodes in two different paths
    cases["read_in_two_groups"] = ([0, 0], [[a], [b]], [(1, 180), (121, 300)])
    g = jm.join(ro, rid, part, cases["read_in_two_groups"][1])
    assert len(np.intersect1d(g[0], g[1])) > 0
    # a one-node path and a path with no node
    cases["one_node"] = ([0], [[(1, 0)]], [(121, 300)])
    cases["no_node"] = ([0, 0, 0], [[], [(2, 0)], []], [(5, 9), (1, 3), (7, 7)])
    # a path that skips an empty block
    gb = w["gap_blocks"]
    assert cnt[gb] > 0 and cnt[gb + 1] == 0 and bp[gb + 1] == 0 and cnt[gb + 2] > 0
    cases["skips_empty_block"] = ([1], [[(gb, 0), (gb + 2, 0)]], [(1, 80)])
    # nodes whose lists have 64, 65 and 129 entries
    for n, blk in w["sized"].items():
        assert cnt[blk] == n and bp[blk] >= 1
        cases[f"list_{n}"] = ([0] * int(bp[blk]), [[(blk, k)] for k in range(int(bp[blk]))], [(1, 2)] * int(bp[blk]))
    cases["lists_all"] = ([0], [[(w["sized"][n], 0) for n in (64, 65, 129)]], [(1, 2)])
    # a window of more than 64 x 64 ids
    bb = w["big_blocks"]
    cases["wide_window"] = ([2, 2], [[(bb, 0), (bb + 1, 0)], [(bb + 1, int(bp[bb + 1]) - 1)]], [(1, 300), (289, 300)])
    lo, hi = jm.windows(ro, rid, cases["wide_window"][1])[0]
    assert hi - lo > 64 * 64, (lo, hi)
    # five contigs in one call, one of them (3) without a path
    sb = w["small_blocks"]
    pc, nodes, ranges = [], [], []
    for name in ("dedupe", "read_in_two_groups", "no_node", "skips_empty_block", "wide_window"):
        c = cases[name]
        pc += c[0]; nodes += c[1]; ranges += c[2]
    order = np.argsort(np.asarray(pc), kind="stable")
    pc = [pc[i] for i in order]; nodes = [nodes[i] for i in order]; ranges = [ranges[i] for i in order]
    pc += [4, 4]; nodes += [[(sb, 0), (sb + 1, 0), (sb + 2, 0)], [(sb + 1, int(bp[sb + 1]) - 1)]]; ranges += [(1, 200), (60, 150)]
    assert sorted(set(pc)) == [0, 1, 2, 4]
    cases["five_contigs"] = (pc, nodes, ranges)
    return cases


CASE_NAMES = ["dedupe", "read_in_two_groups", "one_node", "no_node", "skips_empty_block", "list_64", "list_65", "list_129", "lists_all", "wide_window", "five_contigs"]


def ensure_resident(gpu_ctx, w):
    """The fixture's S1 result, resident: phased again (the same result) if another call ended its residency."""
    try:
        gpu_ctx.join_paths(w["res"], w["contigs"], [], [], []).free()
    except Exception:
        again = w["phase"]()
        assert np.array_equal(again.read_id, w["res"].read_id) and np.array_equal(again.part, w["res"].part) and np.array_equal(again.best_ploidy, w["res"].best_ploidy)
        w["res"] = again
    return w["res"]


@pytest.mark.parametrize("chain_wgs", [0, 1])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case(gpu_ctx, sized, name, chain_wgs):
    assert sorted(sized["cases"]) == sorted(CASE_NAMES)
    res = ensure_resident(gpu_ctx, sized)
    pc, nodes, ranges = sized["cases"][name]
    want = jc.model_groups(res, nodes)
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        hs = gpu_ctx.join_paths(res, sized["contigs"], pc, nodes, ranges)
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    jc.same_as_model(hs.download(), pc, want, ranges, 5, name)
    if name == "five_contigs":
        assert hs.download()[3].n_groups == 0
        t = gpu_ctx.timing()
        assert t["select_ms"] > 0 and t["d2h_ms"] > 0
    hs.free()


def test_no_path_and_no_contig(gpu_ctx, sized):
    res = ensure_resident(gpu_ctx, sized)
    hs = gpu_ctx.join_paths(res, sized["contigs"], [], [], [])
    assert [g.n_groups for g in hs.download()] == [0] * 5
    assert gpu_ctx.haploset_stats(sized["contigs"], haplosets=hs).shape == (0, 4)
    hs.free()


@pytest.mark.parametrize("chain_wgs", [0, 1])
def test_random_contigs(gpu_ctx, rand, chain_wgs):
    res = ensure_resident(gpu_ctx, rand)
    pc, nodes, ranges = jc.random_paths(res, rand["bc"], jc.N_RANDOM, seed=1)
    want = jc.model_groups(res, nodes)
    assert len(nodes) > jc.N_RANDOM and any(len(n) == 0 for n in nodes) and any(len(g) > 64 for g in want)
    gpu_ctx.set_option("chain_wgs", chain_wgs)
    try:
        hs = gpu_ctx.join_paths(res, rand["contigs"], pc, nodes, ranges)
    finally:
        gpu_ctx.set_option("chain_wgs", 0)
    jc.same_as_model(hs.download(), pc, want, ranges, jc.N_RANDOM, "random")
    hs.free()


def test_without_lists_and_around_hap_graph(gpu_ctx, rand):
    """"s1_no_lists" = 1: S1 returns no list (NULL), every other field as before, and the join gives what the lists of the default call give — before floria_hip_hap_graph,
    after it, and twice."""
    base = ensure_resident(gpu_ctx, rand)
    pc, nodes, ranges = jc.random_paths(base, rand["bc"], jc.N_RANDOM, seed=2)
    want = jc.model_groups(base, nodes)
    g0 = gpu_ctx.hap_graph(base)
    gpu_ctx.set_option("s1_no_lists", 1)
    try:
        res = rand["phase"]()
    finally:
        gpu_ctx.set_option("s1_no_lists", 0)
    assert not res.has_lists and len(res.read_id) == 0 and len(res.part) == 0 and base.has_lists
    assert np.array_equal(res.best_ploidy, base.best_ploidy) and np.array_equal(res.read_off, base.read_off) and res.batch_token != base.batch_token
    assert np.array_equal(res.mec.view(np.uint64), base.mec.view(np.uint64)) and np.array_equal(res.ploidies_tried, base.ploidies_tried)
    for when in ("before", "after", "again"):
        hs = gpu_ctx.join_paths(res, rand["contigs"], pc, nodes, ranges)
        jc.same_as_model(hs.download(), pc, want, ranges, jc.N_RANDOM, when + " hap_graph")
        hs.free()
        if when == "before":
            g1 = gpu_ctx.hap_graph(res)
            assert np.array_equal(g1.edge_w, g0.edge_w) and np.array_equal(g1.node_cov.view(np.uint64), g0.node_cov.view(np.uint64))
    rand["res"] = rand["phase"]()                          # (the fixture's result is the one with lists)


def test_stats_on_a_joined_handle(gpu_ctx, sized):
    res = ensure_resident(gpu_ctx, sized)
    pc, nodes, ranges = sized["cases"]["five_contigs"]
    ranges = [(1, 600)] * len(pc)
    hs = gpu_ctx.join_paths(res, sized["contigs"], pc, nodes, ranges)
    gc, groups, rr = jc.listed(hs.download())
    assert gc == pc and any(len(g) == 0 for g in groups) and any(len(g) > 64 for g in groups)
    a = gpu_ctx.haploset_stats(sized["contigs"], haplosets=hs)
    b = gpu_ctx.haploset_stats(sized["contigs"], gc, groups, rr)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.isfinite(b).any()
    hs.free()


def test_refusals(gpu_ctx, hip_lib, sized):
    res = ensure_resident(gpu_ctx, sized)
    cs = sized["contigs"]
    pc, nodes, ranges = sized["cases"]["five_contigs"]
    off = np.zeros(len(nodes) + 1, np.uint64); off[1:] = np.cumsum([len(n) for n in nodes])
    flat = np.asarray([bk for n in nodes for bk in n], np.int64).reshape(-1, 2)
    nb, npart = flat[:, 0].astype(np.uint32), flat[:, 1].astype(np.uint8)
    rg = np.asarray(ranges, np.uint32).reshape(-1)
    pcs = np.asarray(pc, np.uint32)
    n = len(nodes)

    def refused(msg, res_=res, contigs=cs, n_contigs=5, pc_=pcs, off_=off, nb_=nb, np_=npart, rg_=rg, n_=n, token=None, ctx=gpu_ctx):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            ctx.join_paths_raw(res_, contigs, n_contigs, pc_, off_, nb_, np_, rg_, n_, token=token)
        assert ei.value.code == -1 and msg in str(ei.value), str(ei.value)

    # null arguments, each named
    refused("null argument (res)", res_=None)
    refused("null argument (contigs)", contigs=None)
    refused("null argument (path_contig)", pc_=None)
    refused("null argument (node_off)", off_=None)
    refused("null argument (node_block)", nb_=None)
    refused("null argument (node_part)", np_=None)
    refused("null argument (path_range)", rg_=None)
    L = hip_lib.load()
    assert L.floria_hip_join_paths(None, None, None, 0, None, None, None, None, None, 0, None) == -1 and b"null argument (ctx)" in L.floria_hip_last_error()
    cres = hip_lib.capi.CBlockResult()
    assert L.floria_hip_join_paths(gpu_ctx._h, C.byref(cres), None, 0, None, None, None, None, None, 0, None) == -1 and b"null argument (out)" in L.floria_hip_last_error()
    # a foreign token
    refused("no longer resident", token=res.batch_token + 1)
    refused("no longer resident", token=0)
    # a contig of another context; an array that is not the S1 call's
    other = hip_lib.FloriaHip(0)
    try:
        foreign = other.upload(sized["pileups"][4])
        refused("contig 4 belongs to another context", contigs=cs[:4] + [foreign])
        refused("no longer resident", ctx=other)
        foreign.free()
    finally:
        other.close()
    refused("contigs[3] is not the S1 call's", contigs=cs[:3] + [cs[4], cs[3]])
    refused("contigs: 4 given, the S1 call had 5", contigs=cs[:4], n_contigs=4, pc_=np.minimum(pcs, 3))
    # path_contig
    bad = pcs.copy(); bad[-1] = 5
    refused(f"path_contig[{n - 1}] out of range", pc_=bad)
    bad = pcs.copy(); bad[0], bad[1] = 1, 0
    refused("path_contig descends at path 1", pc_=bad)
    # node_off
    bad = off.copy(); bad[0] = 1
    refused("node_off does not start at 0", off_=bad)
    bad = off.copy(); bad[1] = off[2] + 1
    refused("node_off descends at path 1", off_=bad)
    # node_block, node_part (an empty block has no partition), a node of another contig
    bad = nb.copy(); bad[0] = res.n_blocks
    refused("node_block[0] out of range", nb_=bad)
    bad = npart.copy(); bad[0] = int(res.best_ploidy[nb[0]])
    refused("node_part[0] is not below the best ploidy", np_=bad)
    empty = sized["gap_blocks"] + 1
    first_of_1 = int(off[pc.index(1)])
    bad = nb.copy(); bad[first_of_1] = empty
    badp = npart.copy(); badp[first_of_1] = 0
    refused(f"node_part[{first_of_1}] is not below the best ploidy of block {empty}", nb_=bad, np_=badp)
    bad = nb.copy(); bad[0] = sized["small_blocks"]
    badp = npart.copy(); badp[0] = 0
    refused("node_block[0] belongs to another contig than path 0", nb_=bad, np_=badp)
    # nothing of it ended the residency ...
    hs = gpu_ctx.join_paths(res, cs, pc, nodes, ranges)
    jc.same_as_model(hs.download(), pc, jc.model_groups(res, nodes), ranges, 5, "after the refusals")
    # ... an S2 call does: the token is stale
    gc, groups, rr = jc.listed(hs.download())
    gpu_ctx.reassign_batch(cs, gc, groups, rr, EPS)
    refused("no longer resident")
    hs._groups = None
    jc.same_as_model(hs.download(), pc, jc.model_groups(res, nodes), ranges, 5, "the handle after the S2 call")
    hs.free()
