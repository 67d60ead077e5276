"""`-m "not gpu"`: the model of floria_hip_assemble_contigs_ordered (tests/assemble_order_model.py) on the named cases of tests/test_gpu_assemble_order.py:
every expected order is a permutation of its fragment's cell indices, and the cases that exist to tell the merged order from the one-walk order (the order the
library emulates when nobody gives it one) do differ from it — without them the GPU test could pass on a library that ignores how a fragment was merged."""
import numpy as np
import pytest

from tests import assemble_model as am
from tests import assemble_order_model as om


def case_orders(oracle, cases, n_snps):
    names = sorted(cases)
    recs, tables, walked, frags, where = om.world(cases, names, am.grid_table(n_snps), second_contig=am.grid_table(40, start=40, step=9))
    plan = am.build_plan(walked, frags)
    orders, differs = om.expected_orders(oracle, walked, plan)
    place = {int(k): r for r, k in enumerate(plan["order"][0])}          # fragment of the host's list -> read of the sorted contig
    return names, plan, orders, differs, {n: place[where[n]] for n in names}


@pytest.mark.parametrize("cases,n_snps", [om.WORLDS[k] for k in ("hand", "beyond", "rounds")], ids=["hand", "beyond", "rounds"])
def test_expected_orders_are_permutations_and_the_marked_cases_differ_from_the_one_walk_order(oracle_mod, cases, n_snps):
    names, plan, orders, differs, read_of = case_orders(oracle_mod, cases, n_snps)
    assert orders[0] is not None and orders[1] is None, "contig 0 is merged, contig 1 (single-part fragments only) is not"
    p = plan["pileups"][0]
    assert p.n_reads == 2 * len(names)
    for r in range(p.n_reads):
        lo, hi = int(p.read_off[r]), int(p.read_off[r + 1])
        assert sorted(orders[0][lo:hi]) == list(range(hi - lo)), r
    for n in names:
        must, does = cases[n][1], cases[n][2]
        got = bool(differs[0][read_of[n]])
        if must:
            assert got, n + ": the merged order must differ from the one-walk order"
        if does is not None:
            assert got == does, n
    # a single-part fragment's order IS the one-walk order
    singles = [r for r in range(p.n_reads) if r not in set(read_of.values())]
    assert len(singles) == len(names) and not differs[0][singles].any()


def test_the_figures_of_the_two_large_cases(oracle_mod):
    a = oracle_mod.positions_order([np.arange(1, 1793), [5]])
    b = oracle_mod.positions_order([np.arange(1, 1793)])
    assert int((a != b).sum()) == 1783
    x, y = np.arange(1, 2400, 3), np.arange(5000, 7400, 2)
    a = oracle_mod.positions_order([x, y])
    b = oracle_mod.positions_order([np.concatenate([x, y])])
    assert len(a) == 2000 and int((a != b).sum()) == 5
    a = oracle_mod.positions_order([np.arange(1, 8), [3]])
    b = oracle_mod.positions_order([np.arange(1, 8)])
    assert int((a != b).sum()) == 5


def test_the_case_of_two_search_rounds(oracle_mod):
    """both parts beyond one round of assemble_kernel's 64-ary search (more than 65 * 64 = 4 160 cells), interleaved, one stretch of whole windows the first
    part's alone; the figures of its order pinned with the oracle"""
    a, b = (np.asarray(x, np.int64) for x in om.ROUNDS["two_search_rounds"][0])
    assert (len(a), len(b)) == (6067, 4400) and min(len(a), len(b)) > 4160 and max(a.max(), b.max()) <= om.ROUNDS_SNPS
    union = np.union1d(a, b)
    assert len(union) == 6800 and len(np.intersect1d(a, b)) == 3667
    w, (in_a, in_b) = om.merge_windows([a, b])
    assert len(w) == 141 and (np.diff(w) == 64).all() and w[0] == 1
    assert w[(in_a == 64) & (in_b == 0)].tolist() == [5057, 5121], "the windows full of the first part alone"
    assert ((in_a > 0) & (in_b > 0)).sum() == 139, "every other window holds cells of both parts"
    lo, hi = om.ROUNDS_STRETCH
    assert hi - lo >= 64 and np.isin(np.arange(lo, hi), a).all() and not np.isin(np.arange(lo, hi), b).any()
    x = oracle_mod.positions_order([a, b])
    y = oracle_mod.positions_order([union])
    assert sorted(x) == sorted(union.tolist()) and int((x != y).sum()) == 6798
    # the windows of a hand-sized merge, against a plain restatement
    w, (c0, c1) = om.merge_windows([[1, 2], [71, 72, 200]])
    assert w.tolist() == [1, 71, 200] and c0.tolist() == [2, 0, 0] and c1.tolist() == [0, 2, 1]


def test_random_pairs_differ_from_the_one_walk_order_in_a_third_of_the_fragments_at_least(oracle_mod):
    recs, tables, walked, frags = om.random_pairs()
    plan = am.build_plan(walked, frags)
    orders, differs = om.expected_orders(oracle_mod, walked, plan)
    assert all(o is not None for o in orders)
    n = sum(len(d) for d in differs)
    k = sum(int(d.sum()) for d in differs)
    print("%d of %d random pairs differ from the one-walk order" % (k, n))
    assert n == 3000 and 3 * k >= n
