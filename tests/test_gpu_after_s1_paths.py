"""`-m gpu`: the kernels that run after S1 on the code paths they take once an input exceeds a fixed capacity (tests/after_s1_cases.py), against the oracle.

  graph_kernel          histogram and bitonic sort through the HBM pools instead of LDS
  stats_kernel, consensus_kernel, pair_kernel     ranges and spans beyond one trip of 256 positions (64 for the pairs), every way two spans can lie
  reassign_chain_kernel reads of more than 256 cells or with more than 64 candidate groups (the slow path beside the register fast path)
  reassign_kernel       the same inputs forced onto it ("reassign_path"), and more than 64 candidates in reference arithmetic (the x0 loop)

Bar: bit-exact.  array_equal, f64 through view(np.uint64) with NaN matching NaN; no tolerance anywhere.  Every case asserts the regime it is meant for
from what the device returns, as tests/test_after_s1_cases_cpu.py does from the oracle.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import after_s1_cases as M
from tests.test_gpu_parity import _same_f64

pytestmark = pytest.mark.gpu


def _same_groups(go, gg):
    return go.n_groups == gg.n_groups and np.array_equal(go.range, gg.range) and np.array_equal(go.grp_off, gg.grp_off) and np.array_equal(go.grp_read, gg.grp_read)


# ---- 1. hap graph ----------------------------------------------------------------------------------------------------------------------------------
def _device_graph(gpu_ctx, hip_lib, case, res):
    r = gpu_ctx.phase_blocks_batch(res, case.blk_contig, case.blk_start, case.blk_end, hip_lib.make_params(case.eps, case.max_ploidy, case.beam))
    return r, gpu_ctx.hap_graph(r)


def _check_graph(oracle_mod, case, r, g):
    M.assert_graph_regime(case, r.best_ploidy)                          # the device's own best_ploidy puts the call in the intended regime
    assert np.array_equal(np.diff(g.node_off), r.best_ploidy)
    n_edge = 0
    for ci, (ro, cov, ew, idx) in enumerate(M.oracle_graph(oracle_mod, case)):
        assert np.array_equal(ro.best_ploidy, r.best_ploidy[idx]), (case.name, ci)
        b0, b1 = int(idx[0]), int(idx[-1]) + 1                           # the blocks of a contig are consecutive
        lo, hi = int(g.node_off[b0]), int(g.node_off[b1])
        assert np.array_equal(cov.view(np.uint64), g.node_cov[lo:hi].view(np.uint64)), (case.name, "contig", ci, "node cov", cov, g.node_cov[lo:hi])
        elo, ehi = int(g.edge_off[b0]), int(g.edge_off[b1])
        assert np.array_equal(ew, g.edge_w[elo:ehi]), (case.name, "contig", ci, "edge weights", ew, g.edge_w[elo:ehi])
        assert g.pred[b0] == -1
        n_edge += int(ew.sum())
    assert n_edge > 0 and g.edge_w.sum() == n_edge


@pytest.mark.parametrize("name", [n for n in M.GRAPH_CASES if n != "bookkeeping_two_contigs"])
def test_hap_graph_through_the_pools(gpu_ctx, hip_lib, oracle_mod, name):
    case = M.graph_case(name)
    res = [gpu_ctx.upload(p) for p in case.pileups]
    try:
        r, g = _device_graph(gpu_ctx, hip_lib, case, res)
        _check_graph(oracle_mod, case, r, g)
    finally:
        for x in res:
            x.free()


def test_hap_graph_pool_bookkeeping(gpu_ctx, hip_lib, oracle_mod):
    # an empty block that pred skips, a one-node block, two contigs in one batch (pool slices by block index), and the same call once more (pools re-zeroed)
    case = M.graph_case("bookkeeping_two_contigs")
    res = [gpu_ctx.upload(p) for p in case.pileups]
    try:
        r, g = _device_graph(gpu_ctx, hip_lib, case, res)
        _check_graph(oracle_mod, case, r, g)
        assert r.best_ploidy[1] == 0 and r.best_ploidy[4] == 1
        assert list(g.pred[:7]) == [-1, -1, 0, 2, 3, -1, 5]
        r2, g2 = _device_graph(gpu_ctx, hip_lib, case, res)
        _check_graph(oracle_mod, case, r2, g2)
        assert np.array_equal(g.node_cov.view(np.uint64), g2.node_cov.view(np.uint64)) and np.array_equal(g.edge_w, g2.edge_w)
    finally:
        for x in res:
            x.free()


# ---- 2. haploset statistics and HAPQ ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _oracle_stats(name):
    from oracle import oracle
    case = M.stats_case(name)
    st = np.array([oracle.haploset_stats(case.pileup, case.groups[k], *case.ranges[k]) for k in range(len(case.groups))])
    full = oracle.hapq(case.pileup, case.groups, case.ranges, case.snp_pos, case.block_length)
    alone = oracle.hapq(case.pileup, *case.pairs_only(), case.snp_pos, case.block_length)
    return st, full, alone


def _stats_guards(case):
    lens = {hi - lo + 1 for lo, hi in case.ranges if hi >= lo}
    assert set(M.RANGE_LENGTHS) <= lens and any(hi < lo for lo, hi in case.ranges) and any(len(g) == 0 for g in case.groups)
    for groups, ranges in ((case.groups, case.ranges), case.pairs_only()):
        kinds = M.count_pair_kinds(case.pileup, groups, ranges)
        assert all(kinds.get(k, 0) >= 2 for k in M.PAIR_KINDS), kinds
    slo, slen = M.spans_of(case.pileup, case.groups)
    assert (slen > 2 * M.TRIP).any()


@pytest.mark.parametrize("name", M.STATS_CASES)
def test_haploset_stats_beyond_one_trip(gpu_ctx, hip_lib, oracle_mod, name):
    case = M.stats_case(name)
    _stats_guards(case)
    ref = _oracle_stats(name)[0]
    rc = gpu_ctx.upload(case.pileup)
    try:
        st = gpu_ctx.haploset_stats([rc], np.zeros(len(case.groups), np.uint32), case.groups, case.ranges)
    finally:
        rc.free()
    assert st.shape == ref.shape
    for k in range(len(case.groups)):
        assert _same_f64(ref[k], st[k]), (k, case.ranges[k], ref[k], st[k])
    k0 = len(M.RANGE_LENGTHS)
    assert np.isnan(st[k0][1]) and st[k0][3] == 0 and st[k0 + 1][3] == 0 and st[k0 + 2][3] == 0


@pytest.mark.parametrize("name", M.STATS_CASES)
def test_hapq_beyond_one_trip_and_every_span_pair(gpu_ctx, hip_lib, oracle_mod, name):
    case = M.stats_case(name)
    _stats_guards(case)
    _, full, alone = _oracle_stats(name)
    rc = gpu_ctx.upload(case.pileup)
    try:
        for (groups, ranges), (ohq, orel, oavg) in (((case.groups, case.ranges), full), (case.pairs_only(), alone)):
            hq, rel, avg = gpu_ctx.hapq(rc, groups, ranges, case.snp_pos, case.block_length)
            assert np.array_equal(hq, ohq), (hq, ohq)
            assert _same_f64(rel, orel) and _same_f64([avg], [oavg])
    finally:
        rc.free()


def test_hapq_batch_beyond_one_trip(gpu_ctx, hip_lib, oracle_mod):
    # both versions in one call (the 2-allele contig then runs the 4-allele instance), groups of the two contigs interleaved
    cases = [M.stats_case(n) for n in M.STATS_CASES]
    res = [gpu_ctx.upload(c.pileup) for c in cases]
    try:
        gc, groups, ranges = [], [], []
        for k in range(max(len(c.groups) for c in cases)):
            for ci, c in enumerate(cases):
                if k < len(c.groups):
                    gc.append(ci); groups.append(c.groups[k]); ranges.append(c.ranges[k])
        hq, rel, avg = gpu_ctx.hapq_batch(res, gc, groups, ranges, [c.snp_pos for c in cases], cases[0].block_length)
    finally:
        for x in res:
            x.free()
    gc = np.array(gc)
    for ci, name in enumerate(M.STATS_CASES):
        ohq, orel, oavg = _oracle_stats(name)[1]
        assert np.array_equal(hq[gc == ci], ohq), (name, hq[gc == ci], ohq)
        assert _same_f64(rel[gc == ci], orel) and _same_f64([avg[ci]], [oavg])


# ---- 3. S2 -----------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _oracle_s2(name, order_idx, mode=0, eps=M.EPS):
    """oracle.reassign of a case: order_idx -1 = ascending, k = case.orders[k]; shared by the tests, never changed"""
    from oracle import oracle
    case = M.s2_case(name)
    oracle.set_arith_mode(mode)
    try:
        return oracle.reassign(case.pileup, case.groups, case.ranges, eps, read_order=None if order_idx < 0 else case.orders[order_idx])
    finally:
        oracle.set_arith_mode(0)


def _run_paths(gpu_ctx, case, paths, rc=None):
    """every order of the case under every path in `paths` against the oracle"""
    M.assert_s2_regime(case)
    own = rc is None
    rc = gpu_ctx.upload(case.pileup) if own else rc
    try:
        for path in paths:
            gpu_ctx.set_option("reassign_path", path)
            for oi in range(-1, len(case.orders)):
                order = None if oi < 0 else case.orders[oi]
                gg = gpu_ctx.reassign(rc, case.groups, case.ranges, M.EPS, read_order=order)
                assert _same_groups(_oracle_s2(case.name, oi), gg), (case.name, "reassign_path", path, "order", oi)
    finally:
        gpu_ctx.set_option("reassign_path", 0)
        if own:
            rc.free()


@pytest.mark.parametrize("path", (0, 1, 2))
def test_reassign_more_than_64_candidate_groups(gpu_ctx, hip_lib, oracle_mod, path):
    # reads with 1, 2, 63, 64, 65, 127, 128, 129 and 140 candidates: auto = chain kernel (dense), its slow path for nc > 64
    _run_paths(gpu_ctx, M.s2_case("many_candidates"), (path,))


@pytest.mark.parametrize("eps", (0.04, 0.0437))
def test_reassign_more_than_64_candidate_groups_in_reference_arithmetic(gpu_ctx, hip_lib, oracle_mod, eps):
    # reassign_kernel<A, true> folds the candidates 64 per trip: 65..128 candidates take a second trip of the x0 loop, 129 and 140 a third
    case = M.s2_case("many_candidates")
    M.assert_s2_regime(case)
    nc = M.candidate_counts(case)
    assert (nc > 2 * M.CHAIN_FAST_CANDS).any() and ((nc > M.CHAIN_FAST_CANDS) & (nc <= 2 * M.CHAIN_FAST_CANDS)).any()
    rc = gpu_ctx.upload(case.pileup)
    gpu_ctx.set_option("arith", 1)
    try:
        for oi in range(-1, len(case.orders)):
            gg = gpu_ctx.reassign(rc, case.groups, case.ranges, eps, read_order=None if oi < 0 else case.orders[oi])
            assert _same_groups(_oracle_s2(case.name, oi, 1, eps), gg), (eps, "order", oi)
    finally:
        gpu_ctx.set_option("arith", 0)
        rc.free()


@pytest.mark.parametrize("path", (0, 1, 2))
@pytest.mark.parametrize("name", ("long_reads_2_alleles", "long_reads_4_alleles", "long_and_many"))
def test_reassign_reads_of_more_than_256_cells_with_a_choice(gpu_ctx, hip_lib, oracle_mod, name, path):
    # reads of exactly 255, 256, 257, 300 and 650 cells in 2-3 groups each; long_and_many: 257 cells AND 65 groups in one read
    _run_paths(gpu_ctx, M.s2_case(name), (path,))


@pytest.mark.parametrize("name", ("dense_choices", "sparse_choices"))
def test_reassign_forced_paths_on_the_existing_shapes(gpu_ctx, hip_lib, oracle_mod, name):
    # the inputs the suite already runs under auto routing, now on the kernel auto routing does NOT pick as well
    case = M.s2_case(name)
    _run_paths(gpu_ctx, case, (1, 2))
    gpu_ctx.reassign(case.pileup, case.groups, case.ranges, M.EPS)
    nm = int((M.candidate_counts(case) > 1).sum())
    assert gpu_ctx.timing()["jobs"] == nm and (nm * M.DENSE_RULE >= case.pileup.n_reads) == case.dense


def test_reassign_batch_mixes_chain_and_parallel_contigs(gpu_ctx, hip_lib, oracle_mod):
    cases = [M.s2_case(n) for n in M.MIXED_BATCH]
    for c in cases:
        M.assert_s2_regime(c)
    assert [c.dense for c in cases] == [True, False, False, False, True]
    res = [gpu_ctx.upload(c.pileup) for c in cases]
    try:
        for perm in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            gc, groups, ranges = [], [], []
            for slot, ci in enumerate(perm):
                gc += [slot] * len(cases[ci].groups); groups += cases[ci].groups; ranges += cases[ci].ranges
            out = gpu_ctx.reassign_batch([res[ci] for ci in perm], gc, groups, ranges, M.EPS)
            assert len(out) == len(cases)
            for slot, ci in enumerate(perm):
                assert _same_groups(_oracle_s2(cases[ci].name, -1), out[slot]), (perm, cases[ci].name)
            assert out[perm.index(3)].n_groups == 0                      # the contig without groups
    finally:
        for x in res:
            x.free()


# ---- 5. the group arguments the five haploset entry points share ------------------------------------------------------------------------------------------------
def test_bad_group_arguments_are_refused_by_all_five_entry_points_and_a_good_call_follows(gpu_ctx, hip_lib):
    """haploset_stats, haploset_alleles, read_spans, hapq_batch and reassign_batch take the same (contigs, grp_contig, grp_off, grp_read) and make the same four
    memory-safety tests on the host, before any launch: each is given a grp_off that decreases at group 1, a grp_contig of n_contigs, a read id equal to its
    contig's n_reads and a handle of another context, returns -1 with the entry point's message for that fault, and then answers the good groups with the very
    bytes it gave before the refusals."""
    import ctypes as C

    from tests import assemble_model as am
    from tests import pileup_model as pm
    from tests.test_gpu_assemble import free_all, resident
    from tests.test_gpu_mono import random_contig
    from tests.test_gpu_spans import assemble_sp, records_of

    L, capi = hip_lib.load(), hip_lib.capi
    rng = np.random.default_rng(41)
    pileups = [random_contig(rng, 10, 40), random_contig(rng, 12, 50)]
    n_snps = [40, 50]
    up = gpu_ctx.upload_batch(pileups)
    # read_spans answers only contigs that carry positions: the same two pileups through the resident chain
    tables = [am.grid_table(n_snps[0]), am.grid_table(n_snps[1], start=50, step=3)]
    r0, f0 = records_of(pileups[0], tables[0], 0)
    r1, f1 = records_of(pileups[1], tables[1], 1)
    recs = r0 + r1
    plan = am.build_plan(pm.walk_records(recs, tables), [f0, [[i + len(r0) for i in f] for f in f1]])
    assert all(np.array_equal(a.snp, b.snp) and np.array_equal(a.read_off, b.read_off) for a, b in zip(plan["pileups"], pileups))
    summary = resident(gpu_ctx, recs, tables)
    sp = assemble_sp(gpu_ctx, summary, plan, np.zeros(len(plan["part_rec"]), np.uint8))
    other = hip_lib.FloriaHip(0)
    foreign = other.upload(pileups[1])

    good = dict(gc=[0, 1, 1], off=[0, 3, 6, 9], reads=[0, 1, 2, 0, 1, 2, 3, 4, 5], rg=[1, 40, 1, 50, 5, 45])
    pos = [np.ascontiguousarray(100 * np.arange(1, n + 1), np.uint64) for n in n_snps]

    def call(name, handles, gc, off, reads, rg):
        """-> (return code, message, the call's outputs as bytes)"""
        n, ng = len(handles), len(gc)
        arr = (C.c_void_p * n)(*handles)
        gc, off, reads, rg = np.ascontiguousarray(gc, np.uint32), np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(reads, np.uint32), np.ascontiguousarray(rg, np.uint32)
        head = (gpu_ctx._h, arr, C.c_uint32(n), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64), capi.ptr(reads, C.c_uint32), capi.ptr(rg, C.c_uint32), C.c_uint32(ng))
        if name == "haploset_stats":
            outs = [np.zeros((ng, 4), np.float64)]
            rc = L.floria_hip_haploset_stats(*head, capi.ptr(outs[0], C.c_double))
        elif name == "haploset_alleles":
            pos_off = np.zeros(ng + 1, np.uint64)
            pos_off[1:] = np.cumsum(rg[1::2].astype(np.int64) - rg[0::2] + 1)
            outs = [np.zeros((int(pos_off[-1]), 4), np.uint32)]
            rc = L.floria_hip_haploset_alleles(*head, capi.ptr(pos_off, C.c_uint64), capi.ptr(outs[0], C.c_uint32))
        elif name == "read_spans":
            outs = [np.zeros(len(reads), np.uint32), np.zeros(len(reads), np.uint32)]
            rc = L.floria_hip_read_spans(*head, capi.ptr(outs[0], C.c_uint32), capi.ptr(outs[1], C.c_uint32))
        elif name == "hapq_batch":
            pp = (C.POINTER(C.c_uint64) * n)(*[capi.ptr(p, C.c_uint64) for p in pos])
            ns = np.ascontiguousarray(n_snps, np.uint32)
            outs = [np.zeros(ng, np.uint8), np.zeros(ng, np.float64), np.zeros(n, np.float64)]
            rc = L.floria_hip_hapq_batch(*head, pp, capi.ptr(ns, C.c_uint32), C.c_uint64(1000), capi.ptr(outs[0], C.c_uint8), capi.ptr(outs[1], C.c_double), capi.ptr(outs[2], C.c_double))
        else:
            out = C.POINTER(C.POINTER(capi.CGroups))()
            rc = L.floria_hip_reassign_batch(*head, None, None, C.c_double(M.EPS), C.byref(out))
            outs = []
            if rc == 0:
                for i in range(n):
                    g = capi.Groups(out[i].contents)
                    outs += [np.asarray([g.n_groups], np.uint32), g.grp_off, g.grp_read, g.range]
                L.floria_hip_groups_array_free(out, C.c_uint32(n))
        return rc, L.floria_hip_last_error().decode(), b"|".join(o.tobytes() for o in outs)

    try:
        for name in ("haploset_stats", "haploset_alleles", "read_spans", "hapq_batch", "reassign_batch"):
            mine = [c._h for c in (sp if name == "read_spans" else up)]
            rc, msg, want = call(name, mine, **good)
            assert rc == 0 and len(want) > 8, (name, rc, msg)
            bad_reads = list(good["reads"]); bad_reads[0] = pileups[0].n_reads
            faults = (("grp_off decreases", dict(off=[0, 3, 2, 9])),
                      ("grp_contig out of range", dict(gc=[0, 2, 1])),
                      ("group read id out of range", dict(reads=bad_reads)),
                      ("belongs to another context" if name == "read_spans" else "bad contig handle", dict(handles=[mine[0], foreign._h])))
            for needle, change in faults:
                rc, msg, _ = call(name, **dict(dict(good, handles=mine), **change))
                assert rc == -1 and needle in msg, (name, needle, rc, msg)
                rc, msg, again = call(name, mine, **good)
                assert rc == 0 and again == want, (name, "after: " + needle, rc, msg)
    finally:
        foreign.free(); other.close()
        free_all(up, sp); summary.free()
