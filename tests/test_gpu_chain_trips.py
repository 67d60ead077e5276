"""`-m gpu`: the kernels of the resident chain (records -> cells -> realign -> assemble -> set orders -> drop_monomorphic) beyond ONE trip of their loops.  Every
one of them gives a wavefront (or a thread) to a fragment, record or read and strides over the rest once the grid cap of its launch is reached — which no world
of the other test files reaches (8 workgroups per CU: 8 192 wavefronts on 256 CUs).  The test option "chain_wgs" = N caps those grids at N workgroups, and the
one-thread order kernel at N threads, so the existing small worlds send a wavefront through a second, third, .. fragment: over the LDS tables, the scratch
tables, the running counters and the contig index the fragment before left behind.  Also here: a part long enough for a second round of assemble_kernel's 64-ary
search, and mono_order_kernel on a read of more than 128 surviving cells with a host-given order.  Every expectation is the numpy / oracle model of the stage, bit
for bit; the capped call is also compared field for field with the uncapped one."""
import contextlib
import dataclasses
import functools

import numpy as np
import pytest

from tests import assemble_model as am
from tests import assemble_order_model as om
from tests import mono_model as mm
from tests import pileup_model as pm
from tests import pileup_realign_model as rm
from tests import span_model as sm
from tests.test_gpu_assemble import HAND, TABLE, assemble, assert_same_contigs, batch_world, downloads, free_all, hand_world, resident
from tests.test_gpu_assemble_order import assert_same_fields, check_against_the_model, world_of
from tests.test_gpu_mono import EMPTY, assert_same_contigs as assert_same_filtered_contigs, assert_same_result, batch_inputs, take
from tests.test_gpu_pileup import FIELDS, assert_equal_results, device_walk
from tests.test_gpu_pileup_realign import assert_equal as assert_equal_realigned, device_realign
from tests.test_gpu_spans import assemble_sp, assert_words

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def capped(ctx, n):
    """"chain_wgs" = n inside the block (0: the grids as they are), 0 behind it whatever happens"""
    ctx.set_option("chain_wgs", n)
    try:
        yield
    finally:
        ctx.set_option("chain_wgs", 0)


def assert_same_downloads(a, b, what):
    assert sorted(a) == sorted(b), what
    for call in a:
        assert len(a[call]) == len(b[call])
        for c, (x, y) in enumerate(zip(a[call], b[call])):
            assert sorted(x) == sorted(y)
            assert_same_fields(x, y, f"{what}: {call} call, contig {c}, capped against uncapped")


# ---- the three assemble calls on one world ----------------------------------------------------------------------------------------------------------------------
def with_positions(W):
    """a world of world_of's form plus the SEQ_POS words of its plan (every part behind a fragment's first marked as the second mate)"""
    mate = sm.later_parts_mate(W["plan"])
    return dict(W, mate=mate, words=sm.plan_words(W["walked"], W["plan"], mate))


@functools.lru_cache(maxsize=None)
def asm_world(oracle, which):
    """'hand': all hand cases of tests/test_gpu_assemble.py in one contig; 'batch': its three-contig batch -> the form of world_of, computed once, never changed"""
    if which == "hand":
        recs, walked, frags = hand_world(sorted(HAND))
        tables, frags = [TABLE], [frags]
    else:
        recs, tables, walked, frags, _ = batch_world()
    plan = am.build_plan(walked, frags)
    orders, differs = om.expected_orders(oracle, walked, plan)
    return with_positions(dict(recs=recs, tables=tables, walked=walked, plan=plan, orders=orders, differs=differs, want=om.with_orders(plan["pileups"], orders)))


def three_calls(ctx, hip_lib, W, what):
    """the plain call, the ordered call and the call that keeps the positions (assemble_kernel<true, true>, download field 8) on W, each against its model
    -> {call: the downloads of its handles}"""
    plan, pileups = W["plan"], W["plan"]["pileups"]
    out = {"ordered": check_against_the_model(ctx, hip_lib, W, what)}
    s = resident(ctx, W["recs"], W["tables"])
    plain, sp = [], []
    try:
        plain = assemble(ctx, s, plan)
        sp = assemble_sp(ctx, s, plan, W["mate"])
        assert_same_contigs(ctx, plain, pileups, what + ", plain")
        assert_same_contigs(ctx, sp, pileups, what + ", with positions")
        assert_words(sp, W["words"], what)
        out["plain"] = [downloads(g, p.n_reads, p.n_cells) for g, p in zip(plain, pileups)]
        out["positions"] = [dict(downloads(g, p.n_reads, p.n_cells), seq_pos=g.download("seq_pos", p.n_cells)) for g, p in zip(sp, pileups)]
    finally:
        free_all(plain, sp); s.free()
    return out


@functools.lru_cache(maxsize=None)
def uncapped_calls(ctx, hip_lib, oracle, which):
    W = with_positions(world_of(oracle, which)) if which == "rounds" else asm_world(oracle, which)
    return W, three_calls(ctx, hip_lib, W, which)


# ---- (a) assemble under the cap ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("which", ["hand", "batch"])
def test_assemble_calls_under_the_cap(gpu_ctx, hip_lib, oracle_mod, which, cap):
    """4 (cap 1) or 12 (cap 3) wavefronts share all fragments: the second trip of assemble_kernel's fragment loop in its three instances (COUNT, FILL, FILL with
    positions), whose per-wavefront LDS slots, window cursor and first / last words then follow another fragment's"""
    W, free = uncapped_calls(gpu_ctx, hip_lib, oracle_mod, which)
    n_frags = int(W["plan"]["frag_off"][-1])
    n_parts = np.diff(W["plan"]["part_off"])
    assert n_frags > 4 * cap and (n_parts == 1).any() and (n_parts >= 2).any(), "more fragments than wavefronts; straight copies and merges among them"
    assert any(o is not None for o in W["orders"])
    with capped(gpu_ctx, cap):
        got = three_calls(gpu_ctx, hip_lib, W, f"{which}, cap {cap}")
    assert_same_downloads(got, free, f"{which}, cap {cap}")


# ---- (b) set orders under the cap --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [0, 1], ids=["wavefront", "general"])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("which", ["hand", "beyond", "pairs"])
def test_set_orders_under_the_cap(gpu_ctx, hip_lib, oracle_mod, which, cap, general):
    """every fragment's five tables are bound over what the wavefront's (assemble_order_kernel, LDS) or the thread's (assemble_order_general_kernel, HBM scratch:
    at most `cap` threads take all listed fragments) fragment before left in them"""
    W = world_of(oracle_mod, which)
    assert int(W["plan"]["frag_off"][-1]) > 4, "more fragments than one workgroup has wavefronts"
    gpu_ctx.set_option("asm_order_general", general)
    try:
        with capped(gpu_ctx, cap):
            check_against_the_model(gpu_ctx, hip_lib, W, f"{which}, cap {cap}, general {general}")
    finally:
        gpu_ctx.set_option("asm_order_general", 0)


# ---- (c) a part that needs two rounds of the 64-ary search -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1])
def test_parts_beyond_one_round_of_the_search(gpu_ctx, hip_lib, oracle_mod, cap):
    """asm_lower_bound narrows [lo, hi) to step - 1 = ceil(n / 64) - 1 cells per round and stops at 64: only a part of more than 65 * 64 = 4 160 cells sends it
    through a second round.  Both parts of the case are that long, interleave over the whole table, and one stretch belongs to the first part alone."""
    W, free = uncapped_calls(gpu_ctx, hip_lib, oracle_mod, "rounds")
    walked, plan = W["walked"], W["plan"]
    po = plan["part_off"].astype(np.int64)
    two = [f for f in range(len(po) - 1) if po[f + 1] - po[f] == 2]
    assert len(two) == 1
    a, b = (am.record_cells(walked, int(i))[0].astype(np.int64) for i in plan["part_rec"][po[two[0]]:po[two[0] + 1]])
    assert len(a) > 4160 and len(b) > 4160, "a second round of the search in either part"
    w, (in_a, in_b) = om.merge_windows([a, b])
    full = (in_a == 64) & (in_b == 0)
    assert full.any() and w[full].min() > a[0], "a window full of the first part alone, behind the list's first cell (where the search returns before any round)"
    assert ((in_a > 0) & (in_b > 0)).sum() >= len(w) - 5 and len(np.intersect1d(a, b)) > 100, "the parts interleave and share SNPs (the later part's call wins)"
    assert W["differs"][0].sum() == 1, "the merged set order differs from the one-walk order"
    if cap == 0:
        return                                             # (uncapped_calls has checked the three calls against their models)
    with capped(gpu_ctx, cap):
        got = three_calls(gpu_ctx, hip_lib, W, f"rounds, cap {cap}")
    assert_same_downloads(got, free, f"rounds, cap {cap}")


# ---- (d) drop_monomorphic under the cap --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mono_batch():
    """the eight contigs of test_random_batch_from_three_sources and their model, computed once, never changed"""
    eps = 0.03125
    big, mid, gone, wrap = batch_inputs()
    recs, tables, walked, frags, targs = batch_world()
    plan = am.build_plan(walked, frags)
    pileups = [big, plan["pileups"][0], mid, EMPTY, plan["pileups"][1], gone, plan["pileups"][2], wrap]
    counts = [300, len(tables[0].pos), 60, 7, len(tables[1].pos), 24, len(tables[2].pos), 65700]
    want, want_res = mm.drop_batch(pileups, counts, eps)
    return dict(eps=eps, recs=recs, tables=tables, targs=targs, plan=plan, pileups=pileups, counts=counts, want=want, want_res=want_res)


def set_orders_of(hip_lib, contigs, pileups):
    """the set_order of every output contig (None where it carries none)"""
    out = []
    for c, p in zip(contigs, pileups):
        try:
            out.append(c.download("set_order", p.n_cells))
        except hip_lib.FloriaHipError:
            out.append(None)
    return out


@pytest.mark.parametrize("cap", [1, 3])
def test_drop_monomorphic_under_the_cap(gpu_ctx, hip_lib, cap):
    """the second trip of mono_filter_kernel<true> and mono_order_kernel: mono_out_contig steps the contig forward inside a wavefront's stride, over the contig
    without reads (3), the contig that lost all reads (5) and the assembled contig without reads (4)"""
    B = mono_batch()
    want, want_res = B["want"], B["want_res"]
    n_out = [q.n_reads for q in want]
    assert n_out[3] == 0 and n_out[4] == 0 and n_out[5] == 0 and all(n_out[c] > 0 for c in (0, 1, 2, 6, 7)) and sum(n_out) > 4 * cap
    summary = resident(gpu_ctx, B["recs"], B["tables"], table_args=B["targs"])
    asm = assemble(gpu_ctx, summary, B["plan"])
    single = gpu_ctx.upload(B["pileups"][0])
    up = gpu_ctx.upload_batch([B["pileups"][c] for c in (2, 3, 5, 7)])
    handles = [single, asm[0], up[0], up[1], asm[1], up[2], asm[2], up[3]]
    got, free = [], []
    try:
        batch0, res0 = gpu_ctx.drop_monomorphic(handles, B["counts"], B["eps"], with_set_order=True)
        free = take(hip_lib, gpu_ctx, batch0, res0)
        with capped(gpu_ctx, cap):
            batch, res = gpu_ctx.drop_monomorphic(handles, B["counts"], B["eps"], with_set_order=True)
        got = take(hip_lib, gpu_ctx, batch, res)
        assert gpu_ctx.mono_timing()["order_ms"] > 0
        assert_same_result(res, want_res)
        assert_same_filtered_contigs(gpu_ctx, got, want, f"batch, cap {cap}")
        so, so0 = set_orders_of(hip_lib, got, want), set_orders_of(hip_lib, free, want)
        assert sum(x is not None for x in so0) >= 5
        for c, (x, y) in enumerate(zip(so, so0)):
            assert (x is None) == (y is None), c
            if x is not None:
                assert_same_fields({"set_order": x}, {"set_order": y}, f"contig {c}, capped against uncapped")
    finally:
        free_all(got, free, asm, up, [single]); summary.free()


# ---- (e) mono_order_kernel on reads of more than one 64-cell trip --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_read_orders():
    """`big` (reads of 290 and 100 cells) and `mid` (short reads) of the batch above with a host-given set_order — a seeded random permutation per read — and the
    model's outputs carrying the filtered orders (mm.filter_set_order read by read)"""
    eps = 0.03125
    big, mid = batch_inputs()[:2]
    rng = np.random.default_rng(611)
    pileups = [dataclasses.replace(p, set_order=np.concatenate([rng.permutation(int(n)) for n in np.diff(p.read_off)]).astype(np.uint32)) for p in (big, mid)]
    counts = [300, 60]
    want, want_res = mm.drop_batch(pileups, counts, eps)
    off = np.concatenate([[0], np.cumsum(counts)])
    for c, (p, q) in enumerate(zip(pileups, want)):
        mask = want_res["removed"][off[c]:off[c + 1]]
        old = want_res["old_read"][int(want_res["read_off"][c]):int(want_res["read_off"][c + 1])]
        so = []
        for r in range(q.n_reads):
            lo, hi = int(p.read_off[int(old[r])]), int(p.read_off[int(old[r]) + 1])
            so.append(mm.filter_set_order(p.snp[lo:hi], p.set_order[lo:hi], mask))
        q.set_order = np.concatenate(so + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return dict(eps=eps, pileups=pileups, counts=counts, want=want, want_res=want_res)


@pytest.mark.parametrize("cap", [0, 1])
def test_filtered_set_orders_of_long_reads(gpu_ctx, hip_lib, cap):
    """mono_order_kernel takes a read's cells 64 at a time IN SET ORDER and keeps the rank of the next survivor across the trips: a read whose survivors fill more
    than two trips, with removals in its first, a middle and its last trip"""
    L = long_read_orders()
    pileups, want, want_res = L["pileups"], L["want"], L["want_res"]
    big, out = pileups[0], want[0]
    r = int(np.argmax(np.diff(out.read_off)))
    old = int(want_res["old_read"][r])
    lo, hi = int(big.read_off[old]), int(big.read_off[old + 1])
    assert hi - lo == 290 and int(out.read_off[r + 1] - out.read_off[r]) > 128, "the longest read keeps more than 128 cells: its running rank crosses two trips at least"
    cut = want_res["removed"][:300][big.snp[lo:hi].astype(np.int64) - 1][big.set_order[lo:hi].astype(np.int64)] == 1      # the read's cells in set order: removed?
    assert cut[:64].any() and cut[64:256].any() and cut[256:].any(), "removals in the first, a middle and the last trip"
    assert not np.array_equal(big.set_order[lo:hi], np.arange(hi - lo))
    assert max(np.diff(want[1].read_off)) <= 64 and want[1].n_reads > 50, "the second contig: short reads"
    src = gpu_ctx.upload_batch(pileups)
    got = []
    try:
        with capped(gpu_ctx, cap):
            batch, res = gpu_ctx.drop_monomorphic(src, L["counts"], L["eps"], with_set_order=True)
        got = take(hip_lib, gpu_ctx, batch, res)
        assert_same_result(res, want_res)
        assert_same_filtered_contigs(gpu_ctx, got, want, f"long reads, cap {cap}")
        for c, (g, q) in enumerate(zip(got, want)):
            assert_same_fields({"set_order": g.download("set_order", q.n_cells)}, {"set_order": q.set_order}, f"contig {c}, cap {cap}, against filter_set_order")
    finally:
        free_all(got, src)


# ---- (f) the walk and the realignment under the cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["crafted", "sweep"])
def test_walk_under_the_cap(gpu_ctx, which):
    """four wavefronts walk all records: the second trip of pileup_walk_kernel's record loop in both passes (the LDS prefix values, the SNP cursor, the hard-clip
    word of the record before)"""
    if which == "crafted":
        recs, tables = pm.crafted_case()
        want = pm.walk_records(recs, tables)
    else:
        recs, tables, want = pm.random_sweep()
    assert len(recs) > 4 and int(want[0][-1]) > 1000
    free = device_walk(gpu_ctx, recs, tables)
    with capped(gpu_ctx, 1):
        got = device_walk(gpu_ctx, recs, tables)
    assert_equal_results(got, want, recs)
    for name, g, f in zip(FIELDS, got, free):
        assert np.array_equal(g, f), name + ": capped against uncapped"


def test_realign_under_the_cap(gpu_ctx):
    """one workgroup decides, fills and scatters all cells (8 cells, 8 cells and 256 work-list entries per trip), behind a walk of four wavefronts"""
    recs, tables, refs, walked, (want, counts, d) = rm.cached("sweep", None)
    assert counts["cells"] > 8 and counts["scored"] > 256
    free = device_realign(gpu_ctx, recs, tables, refs)
    with capped(gpu_ctx, 1):
        got = device_realign(gpu_ctx, recs, tables, refs)
    assert_equal_realigned(got, want, counts, "cap 1")
    assert got[1] == free[1]
    for name, g, f in zip(FIELDS, got[0], free[0]):
        assert np.array_equal(g, f), name + ": capped against uncapped"


# ---- (g) refusal -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_negative_cap_is_refused_and_a_good_call_works_afterwards(gpu_ctx, hip_lib):
    recs, tables = pm.crafted_case()
    recs = recs[:12]
    want = pm.walk_records(recs, tables)
    for bad in (-1, -(1 << 40)):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.set_option("chain_wgs", bad)
        assert ei.value.code == -1 and "chain_wgs" in str(ei.value)
        assert_equal_results(device_walk(gpu_ctx, recs, tables), want, recs)
    with capped(gpu_ctx, 1):                               # ... and the option itself still takes a good value
        assert_equal_results(device_walk(gpu_ctx, recs, tables), want, recs)
