"""`-m gpu`: records -> cells -> resident contigs on the device: floria_hip_pileup_records_resident against the two pileup entry points,
floria_hip_assemble_contigs (csrc/assemble_kernel.h) field for field against floria_hip_contig_upload_batch of the model's pileups
(tests/assemble_model.py), its refusals, and floria_hip_haploset_alleles against np.add.at."""
import numpy as np
import pytest

from floria_amd.pileup import Pileup
from tests import assemble_model as am
from tests import pileup_model as pm
from tests import pileup_realign_model as rm

pytestmark = pytest.mark.gpu
FIELDS7 = ("read_off", "first", "last", "snp", "cell_aw", "tw", "meta")


def resident(ctx, recs, tables, refs=None, walk=None, table_args=None):
    kw = dict(pm.pack_records(recs, pad=lambda i: i % 4), **(table_args or pm.pack_tables(tables)))
    if refs is not None:
        off, seq = rm.pack_refs(refs)
        kw.update(ref_off=off, ref_seq=seq, walk=walk)
    return ctx.pileup_records_resident(**kw)


def downloads(contig, n_reads, n_cells):
    counts = dict(read_off=n_reads + 1 if n_reads else 0, first=n_reads, last=n_reads, snp=n_cells, cell_aw=n_cells, tw=2 * n_reads, meta=8 * n_reads)
    return {f: contig.download(f, counts[f]) for f in FIELDS7}


def assert_same_contigs(ctx, got, pileups, what=""):
    """every floria_hip_contig_download field of the assembled handles equals that of an upload of the model's pileups"""
    want = ctx.upload_batch(pileups)
    try:
        for c, (g, w, p) in enumerate(zip(got, want, pileups)):
            assert g.n_reads == p.n_reads
            a, b = downloads(g, p.n_reads, p.n_cells), downloads(w, p.n_reads, p.n_cells)
            for f in FIELDS7:
                if not np.array_equal(a[f], b[f]):
                    bad = np.nonzero(a[f] != b[f])[0]
                    raise AssertionError(f"{what} contig {c}: {f} differs in {len(bad)} of {len(a[f])} places, the first at {int(bad[0])}: {int(a[f][bad[0]])} instead of {int(b[f][bad[0]])}")
            # ... and beyond the handle's size nothing is readable, as for an uploaded one
            with pytest.raises(Exception):
                g.download("snp", p.n_cells + 1)
    finally:
        for w in want:
            w.free()


def assemble(ctx, summary, plan):
    return ctx.assemble_contigs(summary, plan["frag_off"], plan["part_off"], plan["part_rec"], set_order=plan["set_order"])


def free_all(*lists):
    for l in lists:
        for c in l:
            c.free()


# ---- (a) the summary ---------------------------------------------------------------------------------------------------------------------------------
def test_summary_equals_both_pileup_entry_points(gpu_ctx):
    recs, tables, refs, walked, model = rm.cached("crafted")
    kw = dict(pm.pack_records(recs, pad=lambda i: i % 4), **pm.pack_tables(tables))
    off, seq = rm.pack_refs(refs)
    plain = gpu_ctx.pileup_records(**kw)
    (real, counts) = gpu_ctx.pileup_records_realign(**kw, ref_off=off, ref_seq=seq)
    for res, want_counts, s in ((plain, dict(cells=int(plain[0][-1]), in_bounds=0, shortcut=0, scored=0, changed=0), resident(gpu_ctx, recs, tables)),
                                (real, counts, resident(gpu_ctx, recs, tables, refs))):
        cell_off, snp, ref_end = res[0], res[1], res[5]
        assert s.n_records == len(recs) and s.token != 0
        assert np.array_equal(s.cell_off, cell_off) and np.array_equal(s.ref_end, ref_end)
        has = cell_off[1:] > cell_off[:-1]
        first = np.where(has, snp[np.minimum(cell_off[:-1], len(snp) - 1).astype(np.int64)], 0)
        last = np.where(has, snp[(np.maximum(cell_off[1:], 1) - 1).astype(np.int64)], 0)
        assert (~has).sum() >= 3 and has.sum() > 100
        assert np.array_equal(s.first_snp, first) and np.array_equal(s.last_snp, last)
        assert s.counts == want_counts
        s.free()
    assert counts["changed"] > 100          # the two routes differ in the alleles they leave on the device; (b) - (d) read those of the walk


# ---- (b) hand-built merges -----------------------------------------------------------------------------------------------------------------------------
N_SNPS = 72          # (the smallest table that holds a single part of 65 cells and 70 one-cell parts)
TABLE = am.grid_table(N_SNPS)


def cells(snps, seed):
    """{snp: (allele, qual)}: alleles 0..3 and qualities with zeros among them, so that the q = 0 / multi-allelic routing of the flatten is on"""
    rng = np.random.default_rng(seed)
    return {int(s): (int(rng.integers(0, 4)), int(rng.choice([0, 1, 13, 37, 60, 255]))) for s in snps}


def hand_cases():
    """name -> (records' cells, fragments as lists of indices into them)"""
    c = {}
    for n in (1, 16, 17, 64, 65):
        c["single_%d" % n] = ([cells(range(3, 3 + n), n)], [[0]])
    c["two_disjoint"] = ([cells(range(2, 12), 1), cells(range(30, 45), 2)], [[0, 1]])
    c["two_interleaved"] = ([cells(range(5, 60, 2), 3), cells(range(6, 60, 2), 4)], [[0, 1]])
    c["two_identical_sets"] = ([cells(range(10, 50), 5), cells(range(10, 50), 6)], [[0, 1]])
    c["two_boundary_overlap"] = ([cells(range(4, 21), 7), cells(range(20, 40), 8)], [[0, 1]])
    c["empty_second"] = ([cells(range(4, 21), 9), {}], [[0, 1]])
    c["empty_first"] = ([{}, cells(range(4, 21), 10)], [[0, 1]])
    c["against_genome_order"] = ([cells(range(40, 60), 11), cells(range(5, 45), 12)], [[0, 1]])
    c["three_first_and_third_share"] = ([cells(range(3, 11), 13), cells(range(20, 30), 14), cells(range(10, 15), 15)], [[0, 1, 2]])
    c["three_share_one"] = ([cells(range(3, 31), 16), cells(range(30, 50), 17), cells([1, 30, 72], 18)], [[0, 1, 2]])
    c["seventy_one_cell_parts"] = ([cells([s], 100 + s) for s in np.random.default_rng(19).permutation(np.arange(1, 71))], [list(range(70))])
    c["wide_gap"] = ([cells([1, 2], 20), cells([71, 72], 21)], [[1, 0]])
    c["same_record_twice"] = ([cells(range(8, 30), 22), cells(range(20, 40), 23)], [[0, 1, 0]])
    return c


HAND = hand_cases()


def hand_world(names):
    """the records of the named cases back to back, with unused records in between -> (records, walked, fragments of the one contig)"""
    recs, frags = [], []
    for name in names:
        rc, fr = HAND[name]
        base = len(recs)
        recs += [am.record_with(TABLE, x, name="%s_%d" % (name, i)) for i, x in enumerate(rc)]
        frags += [[base + i for i in f] for f in fr]
        recs.append(am.record_with(TABLE, cells(range(1, 40), 999), name="unused"))
    return recs, pm.walk_records(recs, [TABLE]), frags


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_merge(gpu_ctx, name):
    recs, walked, frags = hand_world([name])
    plan = am.build_plan(walked, [frags])
    p = plan["pileups"][0]
    assert p.n_reads == 1
    s = resident(gpu_ctx, recs, [TABLE])
    got = assemble(gpu_ctx, s, plan)
    assert_same_contigs(gpu_ctx, got, plan["pileups"], name)
    free_all(got); s.free()


def test_hand_built_merges_together_sorted_and_with_unused_records(gpu_ctx):
    names = sorted(HAND)
    recs, walked, frags = hand_world(names)
    plan = am.build_plan(walked, [frags])
    order = plan["order"][0]
    assert not np.array_equal(order, np.arange(len(order))), "the sort must permute the fragments"
    used = set(int(x) for x in plan["part_rec"])
    assert len(used) < len(recs)
    p = plan["pileups"][0]
    assert (p.qual == 0).any() and (p.allele >= 2).any() and p.n_reads == len(names)
    s = resident(gpu_ctx, recs, [TABLE])
    got = assemble(gpu_ctx, s, plan)
    assert_same_contigs(gpu_ctx, got, plan["pileups"], "all cases")
    # one residency, assembled a second time (another selection): nothing of the first call is left behind
    plan2 = am.build_plan(walked, [frags[::2]])
    got2 = assemble(gpu_ctx, s, plan2)
    assert_same_contigs(gpu_ctx, got2, plan2["pileups"], "every other case")
    free_all(got, got2); s.free()


# ---- (c) a batch ----------------------------------------------------------------------------------------------------------------------------------------
def batch_world():
    rng = np.random.default_rng(2024)
    tables = [am.grid_table(90), am.grid_table(12, start=40, step=9), am.grid_table(130, start=33, step=6)]
    recs = []
    for c in (0, 2):
        n = len(tables[c].pos)
        for i in range(150):
            lo = int(rng.integers(1, n + 1)); hi = min(n, lo + int(rng.integers(0, 70)))
            snps = [s for s in range(lo, hi + 1) if rng.random() < 0.8] if rng.random() < 0.95 else []
            # contig 0: biallelic, no quality 0; contig 2: four alleles, quality 0 among them (the two routings of the flatten in one batch)
            recs.append(am.record_with(tables[c], {s: (int(rng.integers(0, 2 if c == 0 else 4)), int(rng.integers(1 if c == 0 else 0, 60))) for s in snps},
                                       contig=c, name="b%d_%d" % (c, i)))
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]                                                   # the contigs' records interleave
    walked = pm.walk_records(recs, tables)
    frags = [[], [], []]
    for c in (0, 2):
        mine = [i for i, r in enumerate(recs) if r["contig"] == c]
        full = [i for i in mine if walked[0][i + 1] > walked[0][i]]
        for _ in range(60):
            k = int(rng.choice([1] * 14 + [2] * 5 + [3]))
            f = [int(rng.choice(mine)) for _ in range(k)]
            f[int(rng.integers(0, k))] = int(rng.choice(full))
            frags[c].append(f)
    # a SNP table whose first used entry is not entry 0
    t = pm.pack_tables(tables)
    k = 5
    targs = dict(snp_off=t["snp_off"] + np.uint64(k), snp_pos=np.concatenate([np.arange(k, dtype=np.int64), t["snp_pos"]]),
                 alleles=np.concatenate([np.full((k, 4), ord("A"), np.uint8), t["alleles"]]), n_alleles=np.concatenate([np.ones(k, np.uint8), t["n_alleles"]]))
    return recs, tables, walked, frags, targs


def blocks_for(pileups, width=25, step=17):
    bc, bs, be = [], [], []
    for c, p in enumerate(pileups):
        if p.n_reads:
            hi = int(p.last.max())
            for s in range(1, hi + 1, step):
                bc.append(c); bs.append(s); be.append(min(hi, s + width - 1))
    return np.asarray(bc, np.uint32), np.asarray(bs, np.uint32), np.asarray(be, np.uint32)


def assert_same_blocks(a, b):
    for f in ("best_ploidy", "ploidies_tried", "read_off", "read_id", "part"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.mec.view(np.uint64), b.mec.view(np.uint64)), "mec"
    assert a.min_prune_margin == b.min_prune_margin or (np.isnan(a.min_prune_margin) and np.isnan(b.min_prune_margin))


@pytest.mark.parametrize("arith", [0, 1])
def test_batch_of_three_contigs_and_phasing_on_the_assembled_handles(gpu_ctx, hip_lib, arith):
    recs, tables, walked, frags, targs = batch_world()
    plan = am.build_plan(walked, frags, set_order_rng=np.random.default_rng(77) if arith else None)
    pileups = plan["pileups"]
    assert [p.n_reads for p in pileups] == [60, 0, 60]
    assert max(int(x) for x in np.diff(plan["part_off"])) == 3 and (np.diff(plan["part_off"]) == 2).sum() >= 10
    assert (pileups[2].qual == 0).any() and (pileups[2].allele >= 2).any() and not (pileups[0].qual == 0).any() and not (pileups[0].allele >= 2).any()
    s = resident(gpu_ctx, recs, tables, table_args=targs)
    got = assemble(gpu_ctx, s, plan)
    assert_same_contigs(gpu_ctx, got, pileups, "batch")
    bc, bs, be = blocks_for(pileups)
    assert len(bc) > 8
    prm = hip_lib.make_params(0.04, max_ploidy=3)
    want = gpu_ctx.upload_batch(pileups)
    gpu_ctx.set_option("arith", arith)
    try:
        ra = gpu_ctx.phase_blocks_batch(got, bc, bs, be, prm)
        rb = gpu_ctx.phase_blocks_batch(want, bc, bs, be, prm)
    finally:
        gpu_ctx.set_option("arith", 0)
    assert ra.read_off[-1] > 100
    assert_same_blocks(ra, rb)
    free_all(got, want); s.free()


# ---- (d) refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_handle_and_a_usable_context(gpu_ctx, hip_lib):
    recs, tables, walked, frags, targs = batch_world()
    good = am.build_plan(walked, frags, set_order_rng=np.random.default_rng(78))
    s = resident(gpu_ctx, recs, tables, table_args=targs)

    def refused(plan, needle, summary=None):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            assemble(gpu_ctx, summary or s, plan)
        assert ei.value.code == -1 and needle in str(ei.value), str(ei.value)

    def works():
        got = assemble(gpu_ctx, s, good)
        assert_same_contigs(gpu_ctx, got, good["pileups"], "after a refusal")
        free_all(got)

    def variant(**kw):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        p.update(kw)
        return p

    works()
    pr = good["part_rec"].copy(); pr[3] = len(recs)
    refused(variant(part_rec=pr), "names record"); works()
    other = next(i for i, r in enumerate(recs) if r["contig"] == 2)                    # a record of contig 2 in a fragment of contig 0
    pr = good["part_rec"].copy(); pr[0] = other
    refused(variant(part_rec=pr), "lies on contig"); works()
    empty = next(i for i, r in enumerate(recs) if r["contig"] == 0 and walked[0][i + 1] == walked[0][i])
    f = next(f for f in range(60) if good["part_off"][f + 1] - good["part_off"][f] == 2)
    pr = good["part_rec"].copy(); pr[int(good["part_off"][f]):int(good["part_off"][f + 1])] = empty
    refused(variant(part_rec=pr), "have no cell"); works()
    po = good["part_off"].copy(); po[5] = po[4]
    refused(variant(part_off=po), "has no part"); works()
    fo = good["frag_off"].copy(); fo[1] += 1                                            # [0, 61, 60, 120]
    refused(variant(frag_off=fo), "frag_off decreases"); works()
    # two fragments of contig 0 with different spans swapped: the order is checked on the device, with upload's message
    p0 = good["pileups"][0]
    r = next(r for r in range(59) if (p0.first[r], p0.last[r]) != (p0.first[r + 1], p0.last[r + 1]))
    ends = [int(x) for x in good["part_off"]]
    a, b = good["part_rec"][ends[r]:ends[r + 1]], good["part_rec"][ends[r + 1]:ends[r + 2]]
    pr = np.concatenate([good["part_rec"][:ends[r]], b, a, good["part_rec"][ends[r + 2]:]])
    po = good["part_off"].copy(); po[r + 1] = ends[r] + len(b)
    refused(variant(part_rec=pr, part_off=po, set_order=None), "not sorted by Frag::cmp"); works()
    so = good["set_order"].copy(); so[int(p0.read_off[7])] = so[int(p0.read_off[7]) + 1] if p0.read_off[8] - p0.read_off[7] > 1 else 5
    refused(variant(set_order=so), "is not a permutation"); works()
    refused(variant(frag_off=good["frag_off"][:-1], part_off=good["part_off"][:int(good["frag_off"][-2]) + 1]), "contigs"); works()
    # a second pileup call ends the residency
    gpu_ctx.pileup_records(**pm.pack_records(recs[:3]), **targs)
    refused(good, "live residency")
    s2 = resident(gpu_ctx, recs, tables, table_args=targs)
    refused(good, "live residency")                                                    # ... and the old summary stays stale beside a new residency
    got = assemble(gpu_ctx, s2, good)
    assert_same_contigs(gpu_ctx, got, good["pileups"], "new residency")
    free_all(got); s.free(); s2.free()


# ---- (e) allele tables ----------------------------------------------------------------------------------------------------------------------------------
def test_haploset_alleles_equal_a_numpy_histogram_and_leave_the_stats_alone(gpu_ctx):
    rng = np.random.default_rng(5)
    reads0 = [(np.arange(lo, lo + n), rng.integers(0, 2, n), rng.integers(1, 60, n)) for lo, n in ((1, 12), (3, 20), (3, 9), (10, 30), (18, 8), (25, 14))]
    reads0 += [(np.array([20]), np.array([a]), np.array([30])) for a in (0, 1, 2, 3)]          # SNP 20 with all four alleles
    reads0 = [(s[s != 16], a[s != 16], q[s != 16]) if len(s) > 1 else (s, a, q) for s, a, q in reads0]      # SNP 16 uncovered
    reads1 = [(np.arange(lo, lo + n), rng.integers(0, 2, n), rng.integers(0, 60, n)) for lo, n in ((2, 7), (4, 11), (5, 5))]
    pileups = [Pileup.from_reads(reads0), Pileup.from_reads(reads1)]
    all0 = list(range(pileups[0].n_reads))
    groups = [all0, all0, all0[:5], [], all0[2:7], [0, 1, 2], [1]]
    ranges = [(8, 24), (20, 20), (1, 45), (3, 9), (9, 4), (1, 15), (6, 6)]
    grp_contig = [0, 0, 0, 0, 0, 1, 1]
    contigs = gpu_ctx.upload_batch(pileups)
    before = gpu_ctx.haploset_stats(contigs, grp_contig, groups, ranges)
    pos_off, counts = gpu_ctx.haploset_alleles(contigs, grp_contig, groups, ranges)
    after = gpu_ctx.haploset_stats(contigs, grp_contig, groups, ranges)
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    assert list(pos_off) == [0, 17, 18, 63, 70, 70, 85, 86]
    want = np.zeros_like(counts)
    for g, (grp, (lo, hi), c) in enumerate(zip(groups, ranges, grp_contig)):
        p = pileups[c]
        for r in grp:
            s, a, _ = p.read(r)
            m = (s >= lo) & (s <= hi)
            np.add.at(want, (int(pos_off[g]) + (s[m].astype(np.int64) - lo), a[m].astype(np.int64)), 1)
    assert np.array_equal(counts, want)
    row = counts[int(pos_off[0]) + 20 - 8]
    assert (row > 0).all(), "a position with all four alleles"
    assert counts[int(pos_off[0]) + 16 - 8].sum() == 0, "an uncovered position"
    assert counts[int(pos_off[3]):int(pos_off[4])].sum() == 0 and pos_off[5] == pos_off[4]
    p0 = pileups[0]
    assert p0.first.min() < 8 and p0.last.max() > 24, "group 0's range is narrower than its reads on both sides"
    free_all(contigs)
