"""`-m gpu`: floria_hip_assemble_contigs_ordered (csrc/assemble_order_kernel.h) — the set orders of merged fragments derived on the device, against the CPU oracle's
restatement of the reference's containers (tests/assemble_order_model.py): the downloaded set_order itself, the seven other fields against an upload of the model's
pileups carrying that order, the wavefront kernel against the one-thread kernel, S1 in the reference arithmetic at a non-dyadic epsilon, the composition with
floria_hip_drop_monomorphic, and the refusals."""
import functools

import numpy as np
import pytest

from tests import assemble_model as am
from tests import assemble_order_model as om
from tests import mono_model as mm
from tests.helpers import assert_block_results_equal
from tests.test_gpu_assemble import FIELDS7, assemble, assert_same_blocks, blocks_for, downloads, free_all, resident

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def world_of(oracle, which):
    """-> dict(recs, tables, walked, plan, orders, differs, want): computed once per session, never changed"""
    if which == "pairs":
        recs, tables, walked, frags = om.random_pairs()
    else:
        cases, n_snps = om.WORLDS[which]
        recs, tables, walked, frags, _ = om.world(cases, sorted(cases), am.grid_table(n_snps), second_contig=am.grid_table(40, start=40, step=9))
    plan = am.build_plan(walked, frags)
    orders, differs = om.expected_orders(oracle, walked, plan)
    return dict(recs=recs, tables=tables, walked=walked, plan=plan, orders=orders, differs=differs, want=om.with_orders(plan["pileups"], orders))


def ordered(ctx, s, plan):
    return ctx.assemble_contigs_ordered(s, plan["frag_off"], plan["part_off"], plan["part_rec"])


def assert_no_order(hip_lib, contig):
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        contig.download("set_order", 1)
    assert ei.value.code == -1 and "carries no set_order" in str(ei.value)


def assert_same_fields(a, b, what):
    for f in a:
        if not np.array_equal(a[f], b[f]):
            bad = np.nonzero(a[f] != b[f])[0]
            raise AssertionError(f"{what}: {f} differs in {len(bad)} of {len(a[f])} places, the first at {int(bad[0])}: {int(a[f][bad[0]])} instead of {int(b[f][bad[0]])}")


def all_fields(hip_lib, contig, p, carries):
    d = downloads(contig, p.n_reads, p.n_cells)
    if carries:
        d["set_order"] = contig.download("set_order", p.n_cells)
    else:
        assert_no_order(hip_lib, contig)
    return d


def check_against_the_model(ctx, hip_lib, W, what):
    """the ordered call on W against the model; -> the downloads of its handles"""
    plan, orders, want = W["plan"], W["orders"], W["want"]
    s = resident(ctx, W["recs"], W["tables"])
    got = ordered(ctx, s, plan)
    t = ctx.timing()
    ref = ctx.upload_batch(want)
    plain = assemble(ctx, s, dict(plan, set_order=None))
    out = []
    try:
        assert t["pileup_ms"] > 0
        for c, (g, r, pl, p, o) in enumerate(zip(got, ref, plain, want, orders)):
            assert g.n_reads == p.n_reads
            a, b = all_fields(hip_lib, g, p, o is not None), all_fields(hip_lib, r, p, o is not None)
            if o is not None:
                assert_same_fields({"set_order": a["set_order"]}, {"set_order": o}, f"{what} contig {c} against the model")
            assert_same_fields(a, b, f"{what} contig {c} against the upload")
            if o is None:                                  # not merged: what the plain call gives
                assert_same_fields(a, all_fields(hip_lib, pl, p, False), f"{what} contig {c} against the plain call")
            with pytest.raises(Exception):
                g.download("set_order", p.n_cells + 1)
            out.append(a)
    finally:
        free_all(got, ref, plain); s.free()
    return out


# ---- (a) the hand cases, (b) beyond the wavefront kernel's tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hand", "beyond"])
def test_derived_orders_equal_the_model(gpu_ctx, hip_lib, oracle_mod, which):
    W = world_of(oracle_mod, which)
    assert W["orders"][0] is not None and W["orders"][1] is None
    assert W["differs"][0].sum() == sum(1 for v in (om.HAND if which == "hand" else om.BEYOND).values() if v[1]), "the merged orders must differ from the one-walk orders the library would emulate"
    sums = [sum(len(am.record_cells(W["walked"], int(i))[0]) for i in W["plan"]["part_rec"][int(a):int(b)]) for a, b in zip(W["plan"]["part_off"][:-1], W["plan"]["part_off"][1:])]
    assert (max(sums) <= 223) == (which == "hand"), "hand: every fragment within the wavefront kernel's tables; beyond: not"
    check_against_the_model(gpu_ctx, hip_lib, W, which)


# ---- (c) the wavefront kernel against the one-thread kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hand", "beyond"])
def test_the_general_path_gives_the_same_downloads(gpu_ctx, hip_lib, oracle_mod, which):
    W = world_of(oracle_mod, which)
    fast = check_against_the_model(gpu_ctx, hip_lib, W, which)
    gpu_ctx.set_option("asm_order_general", 1)
    try:
        general = check_against_the_model(gpu_ctx, hip_lib, W, which + ", general path")
    finally:
        gpu_ctx.set_option("asm_order_general", 0)
    for c, (a, b) in enumerate(zip(fast, general)):
        assert sorted(a) == sorted(b)
        assert_same_fields(a, b, f"{which} contig {c}, the two paths")


# ---- (d) seeded random pairs -------------------------------------------------------------------------------------------------------------------------------------
def test_random_pairs(gpu_ctx, hip_lib, oracle_mod):
    W = world_of(oracle_mod, "pairs")
    n = sum(len(d) for d in W["differs"]); k = sum(int(d.sum()) for d in W["differs"])
    print("%d of %d pairs differ from the one-walk order" % (k, n))
    assert n == 3000 and 3 * k >= n
    assert all(o is not None for o in W["orders"])
    check_against_the_model(gpu_ctx, hip_lib, W, "pairs")


# ---- (e) S1 in the reference arithmetic on the derived orders ----------------------------------------------------------------------------------------------------
def test_s1_at_a_non_dyadic_epsilon_equals_the_oracle_and_the_uploaded_handles(gpu_ctx, hip_lib, oracle_mod):
    eps = 0.04
    W = world_of(oracle_mod, "pairs")
    want = W["want"]
    s = resident(gpu_ctx, W["recs"], W["tables"])
    got = ordered(gpu_ctx, s, W["plan"])
    ref = gpu_ctx.upload_batch(want)
    bc, bs, be = blocks_for(want, width=25, step=34)
    prm = hip_lib.make_params(eps, max_ploidy=3)
    gpu_ctx.set_option("arith", 1); oracle_mod.set_arith_mode(1)
    try:
        ra = gpu_ctx.phase_blocks_batch(got, bc, bs, be, prm)
        rb = gpu_ctx.phase_blocks_batch(ref, bc, bs, be, prm)
        assert ra.read_off[-1] > 1000
        assert_same_blocks(ra, rb)
        for c in range(len(want)):
            ro = oracle_mod.phase_blocks(want[c], bs[bc == c], be[bc == c], oracle_mod.make_params(eps, max_ploidy=3), threads=8)
            rg = gpu_ctx.phase_blocks(got[c], bs[bc == c], be[bc == c], prm)
            assert_block_results_equal(ro, rg, f"contig {c}")
    finally:
        gpu_ctx.set_option("arith", 0); oracle_mod.set_arith_mode(0)
        free_all(got, ref); s.free()


# ---- (f) composition with drop_monomorphic ------------------------------------------------------------------------------------------------------------------------
def test_drop_monomorphic_with_set_order_on_the_derived_orders(gpu_ctx, hip_lib, oracle_mod):
    from tests.test_gpu_mono import take
    W = world_of(oracle_mod, "pairs")
    want = W["want"]
    counts = [len(t.pos) for t in W["tables"]]
    s = resident(gpu_ctx, W["recs"], W["tables"])
    got = ordered(gpu_ctx, s, W["plan"])
    ref = gpu_ctx.upload_batch(want)
    a_batch, a_res = gpu_ctx.drop_monomorphic(got, counts, 0.03125, with_set_order=True)
    b_batch, b_res = gpu_ctx.drop_monomorphic(ref, counts, 0.03125, with_set_order=True)
    a, b = take(hip_lib, gpu_ctx, a_batch, a_res), take(hip_lib, gpu_ctx, b_batch, b_res)
    try:
        for k in ("read_off", "old_read", "removed"):
            assert np.array_equal(a_res[k], b_res[k]), k
        model, model_res = mm.drop_batch(want, counts, 0.03125)
        assert np.array_equal(a_res["removed"], model_res["removed"])
        for c, (x, y, m) in enumerate(zip(a, b, model)):
            assert x.n_reads == m.n_reads
            assert_same_fields(all_fields(hip_lib, x, m, m.n_reads > 0), all_fields(hip_lib, y, m, m.n_reads > 0), f"filtered contig {c}")
    finally:
        free_all(a, b, got, ref); s.free()


# ---- (g) refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_a_good_call_after_each(gpu_ctx, hip_lib, oracle_mod):
    from tests import pileup_model as pm
    W = world_of(oracle_mod, "hand")
    plan = W["plan"]
    s = resident(gpu_ctx, W["recs"], W["tables"])

    def works(summary):
        got = ordered(gpu_ctx, summary, plan)
        try:
            for g, p, o in zip(got, W["want"], W["orders"]):
                if o is not None:
                    assert np.array_equal(g.download("set_order", p.n_cells), o)
                else:
                    assert_no_order(hip_lib, g)
            with pytest.raises(hip_lib.FloriaHipError) as ei:      # field 8 is still unknown
                hip_lib._check(hip_lib.load().floria_hip_contig_download(got[0]._h, 8, None, 0))
            assert ei.value.code == -1 and "unknown field" in str(ei.value)
        finally:
            free_all(got)

    works(s)
    given = np.concatenate([o if o is not None else np.arange(0, dtype=np.uint32) for o in W["orders"]])
    so = np.zeros(sum(p.n_cells for p in W["want"]), np.uint32)
    so[:len(given)] = given
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        gpu_ctx.assemble_contigs(s, plan["frag_off"], plan["part_off"], plan["part_rec"], set_order=so, _ordered=True)
    assert ei.value.code == -1 and "not both" in str(ei.value)
    works(s)
    # a later pileup call ends the residency: the stale summary is refused, a new one works
    gpu_ctx.pileup_records(**pm.pack_records(W["recs"][:3]), **pm.pack_tables(W["tables"]))
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        ordered(gpu_ctx, s, plan)
    assert ei.value.code == -1 and "live residency" in str(ei.value)
    s2 = resident(gpu_ctx, W["recs"], W["tables"])
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        ordered(gpu_ctx, s, plan)
    assert ei.value.code == -1 and "live residency" in str(ei.value)
    works(s2)
    s.free(); s2.free()
