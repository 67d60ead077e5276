"""The inputs of tests/after_s1_cases.py land in the regimes they are built for: proved here from the oracle and numpy alone (no device), so that a case which
silently stops reaching its code path fails a test that every run executes.  tests/test_gpu_after_s1_paths.py repeats the same guards on what the device returns.
Every guard is an assertion; nothing here skips."""
import numpy as np
import pytest

from tests import after_s1_cases as M


# ---- hap graph: which side of the two capacities of graph_kernel.h every case lies on ---------------------------------------------------------------
@pytest.mark.parametrize("name", M.GRAPH_CASES)
def test_graph_case_regime(oracle_mod, name):
    case = M.graph_case(name)
    best = np.zeros(len(case.blk_start), np.int64)
    n_edges_nonzero = 0
    for ro, cov, ew, idx in M.oracle_graph(oracle_mod, case):
        best[idx] = ro.best_ploidy
        assert len(cov) == int(ro.best_ploidy.sum())
        n_edges_nonzero += int((ew > 0).sum())
    M.assert_graph_regime(case, best)
    assert n_edges_nonzero > 0                                          # consecutive blocks share reads: the edge weights are not all zero
    assert all(2 <= M.n_alleles_of(p) <= 4 for p in case.pileups)


def test_graph_cases_cover_all_four_combinations(oracle_mod):
    seen = set()
    for name in M.GRAPH_CASES:
        case = M.graph_case(name)
        seen.add((case.hist_in_lds, case.sort_in_lds))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    # the sort boundary sits exactly on the capacity: 1024 * 2 cells is the last LDS sort, 1025 * 2 the first one in the pool
    for n, side in ((1024, True), (1025, False)):
        case = M.graph_case(f"biallelic_sort_boundary_{n}")
        assert set((case.blk_end - case.blk_start + 1).tolist()) == {n} and case.sort_in_lds == side
    assert 1024 * 2 == M.GRAPH_SORT_CAP


def test_graph_bookkeeping_case_has_the_blocks_it_is_about(oracle_mod):
    case = M.graph_case("bookkeeping_two_contigs")
    (r0, cov0, ew0, idx0), (r1, cov1, ew1, idx1) = M.oracle_graph(oracle_mod, case)
    bp = r0.best_ploidy
    assert bp[1] == 0 and bp[0] >= 2 and bp[2] >= 2 and bp[4] == 1 and bp[3] >= 1
    assert int(np.diff(r0.read_off)[1]) == 0                            # no read touches the empty block
    # edges of contig 0: 0 -> 2 (the empty block is skipped), 2 -> 3, 3 -> 4; the last one has a single column and is not zero
    assert len(ew0) == bp[0] * bp[2] + bp[2] * bp[3] + bp[3] * bp[4]
    assert ew0[:bp[0] * bp[2]].sum() > 0 and ew0[-int(bp[3] * bp[4]):].sum() > 0
    assert len(case.pileups) == 2 and (r1.best_ploidy >= 2).all()


# ---- haploset statistics and HAPQ: ranges and spans beyond one trip of 256 positions, every kind of span pair -----------------------------------------
@pytest.mark.parametrize("name", M.STATS_CASES)
def test_stats_case_regime(oracle_mod, name):
    case = M.stats_case(name)
    pile = case.pileup
    lens = [hi - lo + 1 for lo, hi in case.ranges[:len(M.RANGE_LENGTHS)]]
    assert tuple(lens) == M.RANGE_LENGTHS
    assert {M.TRIP - 1, M.TRIP, M.TRIP + 1, 2 * M.TRIP - 1, 2 * M.TRIP + 1} <= set(lens) and max(lens) > 5 * M.TRIP
    # the three degenerate groups
    k = len(M.RANGE_LENGTHS)
    assert len(case.groups[k]) == 0
    lo, hi = case.ranges[k + 1]
    assert len(case.groups[k + 1]) > 0 and (pile.last[case.groups[k + 1]] < lo).all()
    assert case.ranges[k + 2][1] < case.ranges[k + 2][0] and len(case.groups[k + 2]) > 0
    assert case.n_length_groups == k + 3
    # statistics that mean something: nearly every position of a range has support (so the later trips of the position loop add to the sums), the LAST
    # position of every range has (so the ragged last trip does), errors are counted, the empty group gives NaN
    for g in range(len(M.RANGE_LENGTHS)):
        st = oracle_mod.haploset_stats(pile, case.groups[g], *case.ranges[g])
        assert st[3] > 0 and st[3] / st[0] > 0.95 * lens[g] and (lens[g] == 1 or st[2] > 0), (g, st)
        last = oracle_mod.haploset_stats(pile, case.groups[g], case.ranges[g][1], case.ranges[g][1])
        assert last[3] > 0, (g, last)
    assert np.isnan(oracle_mod.haploset_stats(pile, case.groups[k], *case.ranges[k])[1])
    assert oracle_mod.haploset_stats(pile, case.groups[k + 1], *case.ranges[k + 1])[3] == 0
    # spans (what consensus_kernel and pair_kernel see) beyond one and two trips
    slo, slen = M.spans_of(pile, case.groups)
    assert (slen > M.TRIP).any() and (slen > 2 * M.TRIP).any() and (slen[:k] % M.TRIP != 0).any()
    # every kind of pair is selected, in the full list and in the list of the crafted pairs alone
    full = M.count_pair_kinds(pile, case.groups, case.ranges)
    alone = M.count_pair_kinds(pile, *case.pairs_only())
    for kind in M.PAIR_KINDS:
        assert full.get(kind, 0) >= 2 and alone.get(kind, 0) == 2, (kind, full, alone)
    assert sum(alone.values()) == 2 * len(M.PAIR_KINDS)                 # crafted pairs alone: every group has exactly one partner
    for kind, (i, j) in case.pair_groups.items():
        got, oi, oj = M.pair_kind(slo, slen, i, j)
        assert got == kind and (kind in ("disjoint",) or max(oi, oj) > 0), (kind, got, oi, oj)
    if name == "four_alleles":                                          # sites where a group holds all four alleles: the 0,2,1,3 order of the inner map
        g = case.groups[len(M.RANGE_LENGTHS) - 1]
        seen = np.zeros((M.STATS_SNPS + 1, 4), bool)
        for r in g:
            s, a, q = pile.read(int(r))
            seen[s, a] = True
        assert seen.all(axis=1).sum() > 50 and len(set(pile.qual.tolist())) == 2 and (pile.qual == 0).any()


@pytest.mark.parametrize("name", M.STATS_CASES)
def test_hapq_moves_with_the_pair_distances(oracle_mod, name):
    # HAPQ of the crafted pairs is below its cap and not all equal: a wrong same / diff count of a pair shows in the number
    case = M.stats_case(name)
    g, r = case.pairs_only()
    hq, rel, avg = oracle_mod.hapq(case.pileup, g, r, case.snp_pos, case.block_length)
    assert hq.max() < 60 and len(set(hq.tolist())) > 2
    i, j = (x - case.n_length_groups for x in case.pair_groups["disjoint"])
    assert hq[i] == hq[j] == hq.max()                                   # disjoint spans: no penalty at all


# ---- S2: candidate counts, read lengths and density, recomputed from the group lists ------------------------------------------------------------------
@pytest.mark.parametrize("name", M.S2_CASES)
def test_s2_case_regime(oracle_mod, name):
    case = M.s2_case(name)
    M.assert_s2_regime(case)
    for g in case.groups:
        assert len(g) == 0 or int(g.max()) < case.pileup.n_reads


def test_s2_cases_differ_in_what_auto_routing_runs(oracle_mod):
    dense = [n for n in M.S2_CASES if M.s2_case(n).dense]
    sparse = [n for n in M.S2_CASES if M.s2_case(n).dense is False]
    assert {"many_candidates", "long_reads_2_alleles", "long_reads_4_alleles", "long_and_many", "dense_choices"} <= set(dense)
    assert {"sparse_choices", "no_choice", "no_groups"} <= set(sparse)
    kinds = [M.s2_case(n).dense for n in M.MIXED_BATCH]
    assert True in kinds and False in kinds                             # the mixed batch launches both kernels in one call
    sp = M.s2_case("sparse_choices")
    assert (M.candidate_counts(sp) > 1).sum() > 0                       # ... and its sparse contig has reads with a choice


def test_s2_many_candidates_ties_are_decided_by_id_and_same(oracle_mod):
    # the visiting order matters and equal qualities give ties on diff: the oracle's result changes with the order
    case = M.s2_case("many_candidates")
    outs = set()
    for order in [None] + case.orders:
        go = oracle_mod.reassign(case.pileup, case.groups, case.ranges, M.EPS, read_order=order)
        outs.add(go.grp_read.tobytes() + go.grp_off.tobytes())
    assert len(outs) > 1
    assert (case.pileup.qual == 20).sum() > case.pileup.n_cells // 3
