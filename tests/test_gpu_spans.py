"""`-m gpu`: read positions on resident contigs.  floria_hip_assemble_contigs_opt with FLORIA_ASM_KEEP_SEQ_POS (csrc/assemble_kernel.h), the SEQ_POS words through
floria_hip_drop_monomorphic (csrc/mono_kernel.h), floria_hip_contig_download field 8 and floria_hip_read_spans (csrc/span_kernel.h), each against the numpy model of
tests/span_model.py; the handles with positions against the plain ones in every other field and in S1; the refusals."""
import ctypes as C

import numpy as np
import pytest

from floria_amd.pileup import Pileup
from tests import assemble_model as am
from tests import mono_model as mm
from tests import pileup_model as pm
from tests import span_model as sm
from tests.test_gpu_assemble import FIELDS7, HAND, TABLE, assemble, assert_same_blocks, batch_world, blocks_for, cells, downloads, free_all, hand_world, resident
from tests.test_gpu_mono import random_contig, take

pytestmark = pytest.mark.gpu


def assemble_sp(ctx, summary, plan, part_mate, **kw):
    return ctx.assemble_contigs(summary, plan["frag_off"], plan["part_off"], plan["part_rec"], set_order=plan["set_order"], keep_seq_pos=True, part_mate=part_mate, **kw)


def assert_fields7_equal(got, want, pileups, what=""):
    for c, (g, w, p) in enumerate(zip(got, want, pileups)):
        a, b = downloads(g, p.n_reads, p.n_cells), downloads(w, p.n_reads, p.n_cells)
        for f in FIELDS7:
            assert np.array_equal(a[f], b[f]), f"{what} contig {c}: {f}"


def assert_words(got, words, what=""):
    for c, (g, w) in enumerate(zip(got, words)):
        have = g.download("seq_pos", len(w))
        if not np.array_equal(have, w):
            bad = np.nonzero(have != w)[0]
            raise AssertionError(f"{what} contig {c}: seq_pos differs in {len(bad)} of {len(w)} places, the first at {int(bad[0])}: {int(have[bad[0]]):#x} instead of {int(w[bad[0]]):#x}")
        with pytest.raises(Exception):
            g.download("seq_pos", len(w) + 1)


def refuses_seq_pos(hip_lib, contig):
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        contig.download("seq_pos", 0)
    assert ei.value.code == -1 and "the contig carries no seq_pos" in str(ei.value)


# ---- (a) hand-built merges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_merge_keeps_positions(gpu_ctx, name):
    recs, walked, frags = hand_world([name])
    plan = am.build_plan(walked, [frags])
    mate = sm.later_parts_mate(plan)
    words = sm.plan_words(walked, plan, mate)
    with_cells = [i for i in frags[0] if walked[0][i + 1] > walked[0][i]]
    if len(with_cells) >= 2:
        assert (words[0] >> 31).any(), "some cell comes from a part marked as the second mate"
    s = resident(gpu_ctx, recs, [TABLE])
    plain = assemble(gpu_ctx, s, plan)
    got = assemble_sp(gpu_ctx, s, plan, mate)
    assert_words(got, words, name)
    assert_fields7_equal(got, plain, plan["pileups"], name)
    free_all(got, plain); s.free()


def test_supplementary_parts_and_the_hard_clip_shift(gpu_ctx):
    # part_mate = NULL: every mate is 0 (what supplementary parts get, file_reader.rs:649-651)
    recs, walked, frags = hand_world(["two_interleaved", "three_share_one"])
    plan = am.build_plan(walked, [frags])
    words = sm.plan_words(walked, plan, None)
    assert not (words[0] >> 31).any()
    s = resident(gpu_ctx, recs, [TABLE])
    got = assemble_sp(gpu_ctx, s, plan, None)
    assert_words(got, words, "no part_mate")
    free_all(got); s.free()
    # a supplementary record (flag 0x800) with a leading hard clip: its cells' seq_pos carry the clip's length
    primary = am.record_with(TABLE, cells(range(2, 20), 41), name="p")
    snps = list(range(15, 40))
    lo, hi = int(TABLE.pos[snps[0] - 1]), int(TABLE.pos[snps[-1] - 1])
    seq = bytearray(b"N" * (hi - lo + 1))
    for k, sn in enumerate(snps):
        seq[int(TABLE.pos[sn - 1]) - lo] = am.BASES[k % 4]
    supp = pm.make_record(lo, [("H", 37), ("M", len(seq)), ("H", 5)], bytes(seq), np.full(len(seq), 20, np.uint8), flag=0x800, name="p")
    recs = [primary, supp]
    walked = pm.walk_records(recs, [TABLE])
    wrong = pm.walk_records(recs, [TABLE], ignore_hard_clip=True)
    assert not np.array_equal(walked[4], wrong[4]) and walked[0][2] - walked[0][1] == len(snps)
    plan = am.build_plan(walked, [[[0, 1]]])
    words = sm.plan_words(walked, plan, np.zeros(2, np.uint8))
    assert (words[0] >= 37).sum() >= len(snps) and not np.array_equal(words[0], sm.plan_words(wrong, plan, np.zeros(2, np.uint8))[0])
    s = resident(gpu_ctx, recs, [TABLE])
    got = assemble_sp(gpu_ctx, s, plan, np.zeros(2, np.uint8))
    assert_words(got, words, "hard clip")
    free_all(got); s.free()


# ---- (b) sorted contigs, batches, S1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
def test_sorted_contig_and_batch_phase_as_the_plain_handles(gpu_ctx, hip_lib, arith):
    worlds = []
    recs, walked, frags = hand_world(sorted(HAND))
    worlds.append((recs, [TABLE], walked, [frags], None))
    recs, tables, walked, frags, targs = batch_world()                                   # three contigs, the middle one empty, snp_off[0] > 0
    assert targs["snp_off"][0] > 0
    worlds.append((recs, tables, walked, frags, targs))
    prm = hip_lib.make_params(0.04, max_ploidy=3)
    for recs, tables, walked, frags, targs in worlds:
        plan = am.build_plan(walked, frags, set_order_rng=np.random.default_rng(79) if arith else None)
        mate = sm.later_parts_mate(plan)
        words = sm.plan_words(walked, plan, mate)
        used = set(int(x) for x in plan["part_rec"])
        assert len(used) < len(recs) and any(not np.array_equal(o, np.arange(len(o))) for o in plan["order"])
        s = resident(gpu_ctx, recs, tables, table_args=targs)
        plain = assemble(gpu_ctx, s, plan)
        got = assemble_sp(gpu_ctx, s, plan, mate)
        assert_words(got, words, "sorted")
        assert_fields7_equal(got, plain, plan["pileups"], "sorted")
        assert any((w >> 31).any() for w in words) and any((w >> 31 == 0).any() for w in words)
        bc, bs, be = blocks_for(plan["pileups"])
        gpu_ctx.set_option("arith", arith)
        try:
            ra = gpu_ctx.phase_blocks_batch(got, bc, bs, be, prm)
            rb = gpu_ctx.phase_blocks_batch(plain, bc, bs, be, prm)
        finally:
            gpu_ctx.set_option("arith", 0)
        assert ra.read_off[-1] > 50
        assert_same_blocks(ra, rb)
        free_all(got, plain); s.free()


def test_both_flags_set_orders_and_positions(gpu_ctx):
    recs, walked, frags = hand_world(sorted(HAND))
    plan = am.build_plan(walked, [frags])
    mate = sm.later_parts_mate(plan)
    words = sm.plan_words(walked, plan, mate)
    n = plan["pileups"][0].n_cells
    s = resident(gpu_ctx, recs, [TABLE])
    ordered = gpu_ctx.assemble_contigs_ordered(s, plan["frag_off"], plan["part_off"], plan["part_rec"])
    both = assemble_sp(gpu_ctx, s, plan, mate, _flags=3)
    so = ordered[0].download("set_order", n)
    assert not np.array_equal(so, np.concatenate([np.arange(k) for k in np.diff(plan["pileups"][0].read_off)]))
    assert np.array_equal(both[0].download("set_order", n), so)
    assert_words(both, words, "both flags")
    assert_fields7_equal(both, ordered, plan["pileups"], "both flags")
    free_all(ordered, both); s.free()


def test_flags_0_and_1_are_the_two_existing_calls(gpu_ctx, hip_lib):
    recs, walked, frags = hand_world(sorted(HAND))
    plan = am.build_plan(walked, [frags])
    n = plan["pileups"][0].n_cells
    s = resident(gpu_ctx, recs, [TABLE])
    args = (s, plan["frag_off"], plan["part_off"], plan["part_rec"])
    plain, ordered = gpu_ctx.assemble_contigs(*args), gpu_ctx.assemble_contigs_ordered(*args)
    f0, f1 = gpu_ctx.assemble_contigs(*args, _flags=0), gpu_ctx.assemble_contigs(*args, _flags=1)
    assert_fields7_equal(f0, plain, plan["pileups"], "flags 0")
    assert_fields7_equal(f1, ordered, plan["pileups"], "flags 1")
    assert np.array_equal(f1[0].download("set_order", n), ordered[0].download("set_order", n))
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        f0[0].download("set_order", n)
    assert "carries no set_order" in str(ei.value)
    for c in (plain[0], ordered[0], f0[0], f1[0]):
        refuses_seq_pos(hip_lib, c)
    free_all(plain, ordered, f0, f1); s.free()


# ---- (c) drop_monomorphic ------------------------------------------------------------------------------------------------------------------------------------
def records_of(p, table, contig, split_every=3):
    """the reads of a Pileup as alignment records; every split_every-th read of three and more cells as TWO overlapping records (the same calls where they
    overlap, so the merged fragment is the read) -> (records, fragments as lists of indices into them)"""
    recs, frags = [], []
    for r in range(p.n_reads):
        s, a, q = p.read(r)
        cl = [(int(x), (int(y), int(z))) for x, y, z in zip(s, a, q)]
        if r % split_every == 0 and len(cl) >= 3:
            k = len(cl) // 3
            recs += [am.record_with(table, dict(cl[:2 * k + 1]), contig=contig, name="r%d" % r), am.record_with(table, dict(cl[k:]), contig=contig, name="r%d" % r)]
            frags.append([len(recs) - 2, len(recs) - 1])
        else:
            recs.append(am.record_with(table, dict(cl), contig=contig, name="r%d" % r))
            frags.append([len(recs) - 1])
    return recs, frags


def mono_world():
    """contig 0: the hand case of tests/mono_model.py (a dropped read, a trimmed read that moves behind a later one); contig 1: random, with a read of 290 cells"""
    tables = [am.grid_table(mm.HAND_SNPS), am.grid_table(300, start=50, step=3)]
    big = random_contig(np.random.default_rng(32), 60, 300, lengths=(290, 100))
    r0, f0 = records_of(mm.hand_pileup(), tables[0], 0)
    r1, f1 = records_of(big, tables[1], 1)
    recs = r0 + r1
    frags = [f0, [[i + len(r0) for i in f] for f in f1]]
    walked = pm.walk_records(recs, tables)
    plan = am.build_plan(walked, frags)
    assert np.array_equal(plan["pileups"][0].snp, mm.hand_pileup().snp) and np.array_equal(plan["pileups"][1].snp, big.snp) and max(np.diff(big.read_off)) == 290
    mate = (np.arange(len(plan["part_rec"])) % 3 == 1).astype(np.uint8)
    return recs, tables, walked, plan, mate, [mm.HAND_SNPS, 300]


def eight(contig, p, with_words=True):
    d = downloads(contig, p.n_reads, p.n_cells)
    if with_words:
        d["seq_pos"] = contig.download("seq_pos", p.n_cells)
    return d


def test_drop_monomorphic_moves_the_positions_with_the_cells(gpu_ctx, hip_lib):
    recs, tables, walked, plan, mate, counts = mono_world()
    err = mm.HAND_ERROR
    words = sm.plan_words(walked, plan, mate)
    want, want_res = mm.drop_batch(plan["pileups"], counts, err)
    want_words = [sm.filter_words(p, w, n, err)[1] for p, w, n in zip(plan["pileups"], words, counts)]
    assert np.array_equal(want_res["removed"][:mm.HAND_SNPS], mm.HAND_MASK) and want_res["n_dropped_reads"] >= 1 and want_res["n_removed_cells"] > 50
    old0 = want_res["old_read"][:want[0].n_reads]
    assert not np.array_equal(old0, np.sort(old0)), "a trimmed read moves behind a later one"
    assert any((w >> 31).any() for w in want_words)
    s = resident(gpu_ctx, recs, tables)
    src = assemble_sp(gpu_ctx, s, plan, mate)
    before = [eight(c, p) for c, p in zip(src, plan["pileups"])]
    batch, res = gpu_ctx.drop_monomorphic(src, counts, err)
    got = take(hip_lib, gpu_ctx, batch, res)
    for k in ("read_off", "old_read", "removed"):
        assert np.array_equal(res[k], want_res[k]), k
    ref = gpu_ctx.upload_batch(want)
    assert_fields7_equal(got, ref, want, "filtered")
    assert_words(got, want_words, "filtered")
    after = [eight(c, p) for c, p in zip(src, plan["pileups"])]
    for a, b in zip(before, after):
        for f in a:
            assert np.array_equal(a[f], b[f]), "the inputs are unchanged: " + f
    # a mixed batch: an input without positions gives an output without
    up = gpu_ctx.upload(plan["pileups"][0])
    batch2, res2 = gpu_ctx.drop_monomorphic([src[1], up], [counts[1], counts[0]], err)
    got2 = take(hip_lib, gpu_ctx, batch2, res2)
    assert_words(got2[:1], want_words[1:], "mixed")
    assert_fields7_equal(got2, [ref[1], ref[0]], [want[1], want[0]], "mixed")
    refuses_seq_pos(hip_lib, got2[1])
    free_all(got, got2, ref, src, [up]); s.free()


# ---- (d) the query ----------------------------------------------------------------------------------------------------------------------------------------------
def span_world():
    """contig 0: reads of 1, 65 and 290 cells (with gaps between cells) and a paired fragment whose right part is the second mate; contig 1: some hand cases"""
    t0 = am.grid_table(300, start=40, step=4)
    c1 = cells([5], 1)
    c65 = cells(range(10, 10 + 130, 2), 2)
    s290 = [s for s in range(3, 300) if s not in (50, 51, 120, 200, 201, 202, 280)]
    c290 = cells(s290, 3)
    assert len(c65) == 65 and len(c290) == 290
    recs = [am.record_with(t0, c1, name="a"), am.record_with(t0, c65, name="b"), am.record_with(t0, c290, name="c"),
            am.record_with(t0, cells(range(20, 41, 2), 4), name="d"), am.record_with(t0, cells(range(60, 81, 2), 5), name="d")]
    frags0 = [[0], [1], [2], [3, 4]]
    n0 = len(recs)
    hrecs, _, hfrags = hand_world(["two_interleaved", "single_17", "wide_gap"])
    recs += [dict(r, contig=1) for r in hrecs]
    frags = [frags0, [[i + n0 for i in f] for f in hfrags]]
    tables = [t0, TABLE]
    walked = pm.walk_records(recs, tables)
    plan = am.build_plan(walked, frags)
    mate = sm.later_parts_mate(plan)
    return recs, tables, walked, plan, mate, [300, len(TABLE.pos)]


def edge_queries(pileups):
    """for every read of every contig: lo before the first cell, on a cell, between two cells, behind the last; the mirror image for hi; hi < lo;
    plus a group without reads and one with all reads of a contig -> (grp_contig, groups, ranges)"""
    gc, groups, ranges = [], [], []
    for c, p in enumerate(pileups):
        for r in range(p.n_reads):
            s = p.read(r)[0].astype(np.int64)
            F, L = int(s[0]), int(s[-1])
            gaps = np.nonzero(np.diff(s) > 1)[0]
            mid = int(s[gaps[len(gaps) // 2]]) + 1 if len(gaps) else None            # a SNP between two cells of the read
            on = int(s[len(s) // 2])
            qs = [(max(1, F - 1), L + 3), (on, L + 3), (L + 1, L + 5), (1, L + 1), (1, on), (1, max(0, F - 1)), (F, L), (on + 1, on), (L, F), (on, on)]
            if mid is not None:
                qs += [(mid, L + 3), (1, mid), (mid, mid)]
            for lo, hi in qs:
                gc.append(c); groups.append([r]); ranges.append((lo, hi))
        gc.append(c); groups.append([]); ranges.append((1, 10))
        gc.append(c); groups.append(list(range(p.n_reads))[::-1]); ranges.append((int(p.first.min()) + 2, int(p.last.max()) - 2))
    return gc, groups, ranges


def check_spans(ctx, contigs, pileups, words, gc, groups, ranges, what):
    left, right = ctx.read_spans(contigs, gc, groups, ranges)
    wl, wr = sm.read_spans(pileups, words, gc, groups, ranges)
    assert len(left) == len(wl) == sum(len(g) for g in groups)
    assert np.array_equal(left, wl), what + ": left"
    assert np.array_equal(right, wr), what + ": right"
    return left, right


def test_read_spans_on_assembled_and_filtered_contigs(gpu_ctx, hip_lib):
    recs, tables, walked, plan, mate, counts = span_world()
    pileups = plan["pileups"]
    words = sm.plan_words(walked, plan, mate)
    assert sorted(int(x) for x in np.diff(pileups[0].read_off)) == [1, 22, 65, 290]
    s = resident(gpu_ctx, recs, tables)
    got = assemble_sp(gpu_ctx, s, plan, mate)
    assert_words(got, words, "span world")
    gc, groups, ranges = edge_queries(pileups)
    left, right = check_spans(gpu_ctx, got, pileups, words, gc, groups, ranges, "edges")
    t = gpu_ctx.timing()
    assert t["pileup_ms"] > 0 and t["d2h_ms"] > 0 and t["total_ms"] >= t["pileup_ms"]
    assert (left == sm.NONE).any() and (right == sm.NONE).any() and ((left == sm.NONE) != (right == sm.NONE)).any()
    # the paired fragment: its right end falls on a cell of the second mate, its left end on one of the first
    pr = next(r for r in range(pileups[0].n_reads) if pileups[0].read_off[r + 1] - pileups[0].read_off[r] == 22)
    l1, r1 = gpu_ctx.read_spans(got, [0], [[pr]], [(1, 300)])
    assert l1[0] >> 31 == 0 and r1[0] >> 31 == 1 and r1[0] != sm.NONE
    # two contigs, several reads per group, seeded random ranges
    rng = np.random.default_rng(90)
    gc, groups, ranges = [], [], []
    for _ in range(2000):
        c = int(rng.integers(0, 2)); n = counts[c]
        gc.append(c); groups.append([int(rng.integers(0, pileups[c].n_reads))])
        lo = int(rng.integers(0, n + 3)); hi = int(rng.integers(0, n + 3)) if rng.random() < 0.3 else lo + int(rng.integers(0, 60))
        ranges.append((lo, hi))
    check_spans(gpu_ctx, got, pileups, words, gc, groups, ranges, "random")
    # the same after drop_monomorphic
    err = 0.3
    want, want_res = mm.drop_batch(pileups, counts, err)
    fwords = [sm.filter_words(p, w, n, err)[1] for p, w, n in zip(pileups, words, counts)]
    assert want_res["n_removed_cells"] > 20 and all(q.n_reads for q in want)
    batch, res = gpu_ctx.drop_monomorphic(got, counts, err)
    out = take(hip_lib, gpu_ctx, batch, res)
    assert_words(out, fwords, "filtered span world")
    gc, groups, ranges = edge_queries(want)
    check_spans(gpu_ctx, out, want, fwords, gc, groups, ranges, "edges after the filter")
    free_all(got, out); s.free()


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_options_and_of_the_query(gpu_ctx, hip_lib):
    L = hip_lib.load()
    capi = hip_lib.capi
    recs, tables, walked, plan, mate, counts = span_world()
    pileups = plan["pileups"]
    words = sm.plan_words(walked, plan, mate)
    s = resident(gpu_ctx, recs, tables)
    fo, po, prc = plan["frag_off"], plan["part_off"], plan["part_rec"]

    def raw_asm(flags, part_mate, null_opts=False, part_rec=None, set_order=None):
        pr_ = np.ascontiguousarray(prc if part_rec is None else part_rec, np.uint32)
        cplan = capi.CFragmentPlan(len(fo) - 1, capi.ptr(fo, C.c_uint64), capi.ptr(po, C.c_uint64), capi.ptr(pr_, C.c_uint32), None if set_order is None else capi.ptr(set_order, C.c_uint32))
        pm_ = None if part_mate is None else np.ascontiguousarray(part_mate, np.uint8)
        opts = capi.CAssembleOptions(flags, None if pm_ is None else capi.ptr(pm_, C.c_uint8))
        hs = (C.c_void_p * 2)(0xdead, 0xdead)
        rc = L.floria_hip_assemble_contigs_opt(gpu_ctx._h, s._p, C.byref(cplan), None if null_opts else C.byref(opts), hs)
        return rc, L.floria_hip_last_error().decode(), hs

    def asm_refused(needle, *a, **kw):
        rc, msg, hs = raw_asm(*a, **kw)
        assert rc == -1 and needle in msg, (rc, msg)
        assert not hs[0] and not hs[1], "no handle"
        got = assemble_sp(gpu_ctx, s, plan, mate)                                       # ... and a good call on the same context and residency
        assert_words(got, words, "after: " + needle)
        free_all(got)

    asm_refused("null argument", 2, None, null_opts=True)
    asm_refused("unknown flag bits", 4, None)
    asm_refused("unknown flag bits", 0x80000002, None)
    asm_refused("without FLORIA_ASM_KEEP_SEQ_POS", 0, mate)
    asm_refused("without FLORIA_ASM_KEEP_SEQ_POS", 1, mate)
    bad = mate.copy(); bad[len(bad) - 2] = 2
    asm_refused("part_mate of part %d is 2" % (len(bad) - 2), 2, bad)
    pr_bad = prc.copy(); pr_bad[1] = len(recs)
    asm_refused("names record", 2, mate, part_rec=pr_bad)
    so = np.concatenate([np.arange(k, dtype=np.uint32) for p in pileups for k in np.diff(p.read_off)])
    asm_refused("give the order or ask for it", 3, mate, set_order=so)

    got = assemble_sp(gpu_ctx, s, plan, mate)
    plain = assemble(gpu_ctx, s, plan)
    good = ([0, 1], [[0, 1], [2]], [(1, 300), (1, 72)])

    def raw_spans(ctx, handles, gc, off, reads, rng_, n_groups, null=()):
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        a = dict(gc=np.ascontiguousarray(gc, np.uint32), off=np.ascontiguousarray(off, np.uint64), reads=np.ascontiguousarray(reads, np.uint32), rng=np.ascontiguousarray(rng_, np.uint32).reshape(-1))
        left, right = np.zeros(len(reads) + 1, np.uint32), np.zeros(len(reads) + 1, np.uint32)
        p = lambda k, t: None if k in null else capi.ptr(a[k], t)
        rc = L.floria_hip_read_spans(ctx._h, None if "contigs" in null else arr, C.c_uint32(len(handles)), p("gc", C.c_uint32), p("off", C.c_uint64), p("reads", C.c_uint32), p("rng", C.c_uint32),
                                     C.c_uint32(n_groups), None if "left" in null else capi.ptr(left, C.c_uint32), None if "right" in null else capi.ptr(right, C.c_uint32))
        return rc, L.floria_hip_last_error().decode()

    hs = [got[0]._h, got[1]._h]
    base = dict(handles=hs, gc=[0, 1], off=[0, 2, 3], reads=[0, 1, 2], rng_=[1, 300, 1, 72], n_groups=2)

    def span_refused(needle, ctx=gpu_ctx, null=(), **kw):
        rc, msg = raw_spans(ctx, **dict(base, **kw), null=null)
        assert rc == -1 and needle in msg, (rc, msg)
        check_spans(gpu_ctx, got, pileups, words, *good, "after: " + needle)         # ... and a good call afterwards

    assert raw_spans(gpu_ctx, **base)[0] == 0
    for k in ("contigs", "gc", "off", "reads", "rng", "left", "right"):
        span_refused("null argument", null=(k,))
    span_refused("null argument", handles=[got[0]._h, None])
    other = hip_lib.FloriaHip(0)
    try:
        span_refused("another context", ctx=other)
    finally:
        other.close()
    span_refused("the contig carries no seq_pos", handles=[got[0]._h, plain[1]._h])
    span_refused("grp_contig out of range", gc=[0, 2])
    span_refused("does not start at 0", off=[1, 2, 3])
    span_refused("grp_off decreases", off=[0, 2, 1])
    span_refused("group read id out of range", reads=[0, pileups[0].n_reads, 0])
    span_refused("group read id out of range", reads=[0, 1, pileups[1].n_reads])
    # no group, or groups without reads, are no error
    l0, r0 = gpu_ctx.read_spans(got, [], [], [])
    assert len(l0) == 0 and len(r0) == 0
    l0, r0 = gpu_ctx.read_spans(got, [0, 1], [[], []], [(1, 5), (2, 9)])
    assert len(l0) == 0
    free_all(got, plain); s.free()
