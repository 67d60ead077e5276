"""Model of floria_hip_assemble_contigs_ordered for the tests: the set_order every read of a merged contig carries, from tests/assemble_model.py's merged
pileups and the CPU oracle's restatement of the reference's containers (oracle.set_order_of -> positions_order, oracle/floria_oracle.cpp).  A contig is merged
when one of its fragments has two or more parts with cells; the other contigs carry no order (None).

Also here: the named hand cases both test files use (parts as lists of SNP indices, merge order), the two cases beyond the wavefront kernel's tables, the
case whose parts are long enough for a second round of assemble_kernel's search, and the seeded random pairs."""
import dataclasses

import numpy as np

from tests import assemble_model as am
from tests import pileup_model as pm


def expected_orders(oracle, walked, plan):
    """-> (per contig: uint32 set_order over the contig's merged cells | None, per contig: bool per fragment "differs from the one-walk order")"""
    orders, differs = [], []
    for c, p in enumerate(plan["pileups"]):
        f0 = int(plan["frag_off"][c])
        so, df, merged_contig = [], [], False
        for r in range(p.n_reads):
            parts = plan["part_rec"][int(plan["part_off"][f0 + r]):int(plan["part_off"][f0 + r + 1])]
            segs = [s for s in (am.record_cells(walked, int(i))[0] for i in parts) if len(s)]
            merged_contig = merged_contig or len(segs) >= 2
            snps = p.read(r)[0]
            so.append(oracle.set_order_of(snps, segs))
            df.append(not np.array_equal(so[-1], oracle.set_order_of(snps, [snps])))
        orders.append(np.concatenate(so + [np.zeros(0, np.uint32)]).astype(np.uint32) if merged_contig else None)
        differs.append(np.asarray(df, bool))
    return orders, differs


def with_orders(pileups, orders):
    """copies of the pileups that carry the orders (None: no set_order)"""
    return [dataclasses.replace(p, set_order=None if o is None else o.copy()) for p, o in zip(pileups, orders)]


def cells(snps, seed):
    """{snp: (allele, qual)} with alleles 0..3 and qualities with zeros among them"""
    rng = np.random.default_rng(seed)
    return {int(s): (int(rng.integers(0, 4)), int(rng.choice([0, 1, 13, 37, 60, 255]))) for s in snps}


R = lambda a, b, s=1: list(range(a, b, s))

# name -> (the parts' SNPs in merge order, an int = the part of that index once more; must the order differ from the one-walk order; does it — pinned with the oracle)
HAND = {
    "k7_plus_3": ([R(1, 8), [3]], True, True),
    "k14_plus_9": ([R(1, 15), [9]], True, True),
    "k28_plus_9": ([R(1, 29), [9]], True, True),
    "k56_plus_9": ([R(1, 57), [9]], True, True),
    "k3_plus_2": ([[1, 2, 3], [2]], True, True),
    "k3_plus_4": ([[1, 2, 3], [4]], False, False),
    "k7_plus_9": ([R(1, 8), [9]], False, False),
    "k3_plus_40_43": ([[3, 4, 5], R(40, 44)], True, True),
    "k7_plus_100_106": ([R(1, 8), R(100, 107)], True, True),
    "two_disjoint": ([R(2, 12), R(30, 45)], True, True),
    "two_identical_sets": ([R(10, 50), R(10, 50)], True, True),
    "wider_than_the_table": ([R(1, 2000, 97), R(50, 2000, 89)], True, True),
    "empty_first": ([[], R(4, 21)], False, False),
    "empty_second": ([R(4, 21), []], False, False),
    "three_parts": ([R(3, 11), R(20, 30), R(10, 15)], False, False),
    "seventy_one_cell_parts": ([[int(s)] for s in np.random.default_rng(19).permutation(np.arange(1, 71))], False, False),
    "same_record_twice": ([R(8, 30), R(20, 40), 0], False, False),
}
BEYOND = {
    "k1792_plus_5": ([R(1, 1793), [5]], True, True),
    "two_thousand_keys": ([R(1, 2400, 3), R(5000, 7400, 2)], True, True),
}
# one fragment of two parts of more than 4 160 cells each: assemble_kernel's 64-ary search of a part's SNP list (asm_lower_bound) narrows a range to step - 1
# cells per round, so only such a part sends it through a second round.  On a table of 9 000 SNPs no part has a SNP that is a multiple of 4; of every 12 SNPs
# the first part has those congruent to 2 3 5 6 7 9 10 11, the second those congruent to 1 2 5 6 9 10: both have cells in every 64-SNP window, and they share
# five SNPs of every 12.  SNPs 5 000 .. 5 199 belong to the first part alone, ALL of them: one whole window [w, w + 64) of the merge at least lies inside the
# stretch, full of that part, at an i0 that two rounds found.  The set order differs from the one-walk order: 6 100 + 2 200 reserved keys outgrow the first part's
# 8 192 buckets, which hold the 6 800 merged keys of a one-walk set.
ROUNDS_SNPS = 9000
ROUNDS_STRETCH = (5000, 5200)
_in_stretch = lambda s: ROUNDS_STRETCH[0] <= s < ROUNDS_STRETCH[1]
ROUNDS = {
    "two_search_rounds": ([[s for s in range(1, ROUNDS_SNPS + 1) if _in_stretch(s) or s % 12 in (2, 3, 5, 6, 7, 9, 10, 11)],
                           [s for s in range(1, ROUNDS_SNPS + 1) if not _in_stretch(s) and s % 12 in (1, 2, 5, 6, 9, 10)]], True, True),
}
# world name -> (cases, SNPs of contig 0's table): what both test files build with world()
WORLDS = {"hand": (HAND, 2000), "beyond": (BEYOND, 7400), "rounds": (ROUNDS, ROUNDS_SNPS)}


def merge_windows(parts):
    """the 64-SNP windows assemble_kernel's merge visits for parts given as ascending SNP arrays: the first starts at the smallest SNP of any part, the next at
    the smallest SNP at or behind w + 64 that any part has -> (window starts, per part: its cells inside every window)"""
    parts = [np.asarray(p, np.int64) for p in parts]
    u = np.unique(np.concatenate(parts))
    w = [int(u[0])]
    while True:
        k = int(np.searchsorted(u, w[-1] + 64))
        if k >= len(u):
            break
        w.append(int(u[k]))
    w = np.asarray(w, np.int64)
    return w, [np.searchsorted(p, w + 64) - np.searchsorted(p, w) for p in parts]


def world(cases, names, table, singles=((5, 9), (1, 40), (60, 61)), second_contig=None):
    """the named cases as fragments of contig 0, single-part fragments among them, and (second_contig: a table) a contig 1 of single-part fragments only
    -> (records, tables, walked, fragments per contig, fragment index of every name in contig 0's list)"""
    recs, frags, where = [], [], {}
    for k, name in enumerate(names):
        parts = cases[name][0]
        base = len(recs)
        own = [x for x in parts if not isinstance(x, int)]
        recs += [am.record_with(table, cells(x, 1000 * k + i), name="%s_%d" % (name, i)) for i, x in enumerate(own)]
        idx, n = [], 0
        for x in parts:
            if isinstance(x, int): idx.append(base + x)
            else: idx.append(base + n); n += 1
        where[name] = len(frags)
        frags.append(idx)
        lo, hi = singles[k % len(singles)]
        recs.append(am.record_with(table, cells(range(lo, hi), 77 + k), name="single_%d" % k))
        frags.append([len(recs) - 1])
    tables, per = [table], [frags]
    if second_contig is not None:
        tables.append(second_contig)
        n = len(second_contig.pos)
        mine = []
        for k in range(5):
            recs.append(am.record_with(second_contig, cells(range(1 + k, min(n, 9 + 3 * k) + 1), 500 + k), contig=1, name="c1_%d" % k))
            mine.append([len(recs) - 1])
        per.append(mine)
    return recs, tables, pm.walk_records(recs, tables), per, where


def random_pairs(n_pairs=3000, n_snps=90, seed=4242):
    """paired reads of 1-7 cells per mate on three contigs of n_snps SNPs (every sixth SNP with one allele only: something for --ignore-monomorphic) -> (records, tables, walked, fragments per contig)"""
    rng = np.random.default_rng(seed)
    tables = [am.grid_table(n_snps), am.grid_table(n_snps, start=40, step=9), am.grid_table(n_snps, start=33, step=6)]
    recs, frags = [], [[], [], []]
    for i in range(n_pairs):
        c = i % 3
        pair = []
        for m in range(2):
            k = int(rng.integers(1, 8))
            lo = int(rng.integers(1, n_snps - 12))
            snps = np.sort(rng.choice(np.arange(lo, lo + 12), size=k, replace=False))
            recs.append(am.record_with(tables[c], {int(s): (int(rng.integers(0, 2)) if s % 6 else 0, int(rng.integers(1, 60))) for s in snps}, contig=c, name="p%d_%d" % (i, m)))
            pair.append(len(recs) - 1)
        frags[c].append(pair)
    return recs, tables, pm.walk_records(recs, tables), frags
