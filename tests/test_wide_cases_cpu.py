"""The worlds of tests/wide_cases.py on the CPU: the shapes tests/test_gpu_wide.py relies on, and what moving a pileup along its contig does to the oracle.

  * canonical arithmetic (mode 0): a moved world gives the same bits;
  * reference arithmetic (mode 1) at a non-dyadic epsilon: it does not - the emulated hash containers are keyed by the absolute SNP index - so the moved
    worlds are new inputs for that mode, not copies;
  * the Python restatement (oracle/py_restatement.py) equals the oracle on a world that straddles SNP index 65 536.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import wide_cases as wc
from tests.helpers import assert_block_results_equal
from tests.test_py_restatement import compare

SEEDS = range(6)               # the seeds tests/test_gpu_wide.py runs


def run(w, eps, mode=0):
    oracle.set_arith_mode(mode)
    try:
        return oracle.phase_blocks(w.pile, w.s, w.e, oracle.make_params(eps, w.P, w.B), threads=8)
    finally:
        oracle.set_arith_mode(0)


def identical(a, b):
    try:
        assert_block_results_equal(a, b)
    except AssertionError:
        return False
    return a.min_prune_margin == b.min_prune_margin


def test_shifted_moves_cells_reads_and_blocks():
    w = wc.dup_world(0)
    m = wc.shifted(w, wc.K_CHROM)
    assert np.array_equal(m.pile.snp.astype(np.int64) - w.pile.snp, np.full(w.pile.n_cells, wc.K_CHROM))
    assert np.array_equal(m.pile.first.astype(np.int64) - w.pile.first, np.full(w.pile.n_reads, wc.K_CHROM))
    assert np.array_equal(m.pile.last.astype(np.int64) - w.pile.last, np.full(w.pile.n_reads, wc.K_CHROM))
    assert np.array_equal(m.s.astype(np.int64) - w.s, [wc.K_CHROM] * 2) and np.array_equal(m.e.astype(np.int64) - w.e, [wc.K_CHROM] * 2)
    assert np.array_equal(m.pile.read_off, w.pile.read_off) and np.array_equal(m.pile.allele, w.pile.allele) and np.array_equal(m.pile.qual, w.pile.qual)
    assert int(w.pile.snp.min()) >= 1 and (wc.K_FAR, wc.K_CHROM) == (3 * 65536 + 1, 5_000_000)


@pytest.mark.parametrize("extra,alleles", [(0, 2), (1, 2), (0, 4)])
def test_span_limit_world_has_the_span_it_claims(extra, alleles):
    w = wc.span_limit_world(extra, alleles)
    pos0, span, ids = wc.block_extent(w.pile, int(w.s[0]), int(w.e[0]))
    assert span == 65536 + extra and pos0 == int(w.s[0]) and pos0 + span - 1 == int(w.e[0])
    assert len(ids) == w.pile.n_reads == 900                                                  # no read is left out: none spans more than 10 001 SNPs
    cells = np.diff(w.pile.read_off)
    assert cells.min() >= 2 and cells.max() <= 40
    assert int(w.pile.allele.max()) == alleles - 1
    if extra == 0:
        assert wc.block_extent(wc.shifted(w, wc.K_FAR).pile, int(w.s[0]) + wc.K_FAR, int(w.e[0]) + wc.K_FAR)[:2] == (pos0 + wc.K_FAR, 65536)


def test_long_world_reads_on_both_sides_of_every_threshold():
    w = wc.long_world()
    p = w.pile
    cells = np.diff(p.read_off.astype(np.int64))
    span = p.last.astype(np.int64) - p.first + 1
    assert p.n_reads == 36 and cells.max() >= 10001
    for n in wc.LONG_SPANS:
        assert np.count_nonzero((span == n) & (cells == n)) == 6                              # dense: as many cells as SNPs
    assert (cells < 4096).any() and (cells == 4096).any() and (cells > 4096).any()
    assert np.count_nonzero(span == 6000) == 6 and np.all(cells[span == 6000] == 300)
    out = np.nonzero(span == 10002)[0]
    for b in range(2):
        pos0, sp, ids = wc.block_extent(p, int(w.s[b]), int(w.e[b]))
        assert len(ids) == 30 and not np.isin(out, ids).any() and np.isin(np.nonzero(span == 10001)[0], ids).all()
        assert sp > 2600
    k = 65536 - 6000
    pos0, sp, _ = wc.block_extent(wc.shifted(p, k), int(w.s[0]) + k, int(w.e[0]) + k)
    assert pos0 < 65536 <= pos0 + sp - 1


@pytest.mark.parametrize("kind", ["dup", "medium"])
def test_k_wrap_puts_a_block_across_index_65536(kind):
    for seed in SEEDS:
        w = wc.dup_world(seed) if kind == "dup" else wc.medium_world(seed)
        w = wc.shifted(w, wc.k_wrap(w))
        across = 0
        for b in range(len(w.s)):
            pos0, span, ids = wc.block_extent(w.pile, int(w.s[b]), int(w.e[b]))
            across += len(ids) > 0 and pos0 < 65536 <= pos0 + span - 1
        assert across >= 1, (kind, seed)


def test_medium_worlds_cover_four_alleles_and_q0():
    ws = [wc.medium_world(seed) for seed in SEEDS]
    assert sum(int(w.pile.allele.max()) == 3 for w in ws) == 2 and sum(bool((w.pile.qual == 0).any()) for w in ws) >= 1
    assert all(150 <= w.pile.n_reads <= 500 and 40 <= w.S <= 300 for w in ws)


@pytest.mark.parametrize("kind", ["dup", "medium"])
def test_canonical_arithmetic_does_not_see_the_offset(kind):
    for seed in SEEDS:
        w = wc.dup_world(seed) if kind == "dup" else wc.medium_world(seed)
        for eps in (0.03125, 0.04):
            r = run(w, eps)
            for name, k in wc.offsets(w).items():
                assert identical(r, run(wc.shifted(w, k), eps)), (kind, seed, eps, name)


def test_canonical_arithmetic_does_not_see_the_offset_long_and_wide():
    w = wc.long_world()
    assert identical(run(w, 0.04), run(wc.shifted(w, 65536 - 6000), 0.04))
    for alleles in (2, 4):
        w = wc.span_limit_world(0, alleles)
        assert identical(run(w, 0.04), run(wc.shifted(w, wc.K_FAR), 0.04))


def test_reference_arithmetic_sees_the_offset():
    """... so the moved worlds of the reference-arithmetic tests on the device are inputs that mode has not met: at least a quarter of them at K_FAR."""
    differ = sum(not identical(run(w, 0.04, 1), run(wc.shifted(w, wc.K_FAR), 0.04, 1)) for w in (wc.medium_world(seed) for seed in SEEDS))
    assert 4 * differ >= len(SEEDS), differ


def test_python_restatement_across_index_65536():
    """The second restatement of S1 against the oracle on worlds moved by K_WRAP, in the modes tests/test_py_restatement.py compares: canonical at a dyadic
    epsilon, running sums in ascending key order (mode 2) at 0.04.  The block [1, last SNP] takes every read, as the unmoved worlds' first block does."""
    for w in (wc.dup_world(2), wc.medium_world(5, small=True)):
        k = wc.k_wrap(w)
        m = wc.shifted(w.pile, k)
        assert int(m.first.min()) < 65536 <= int(m.last.max())
        for eps, mode in ((0.03125, 0), (0.04, 2)):
            ro = compare(m, w.S + k, w.P, w.B, eps, mode)
            assert int(ro.read_off[-1]) == w.pile.n_reads and ro.best_ploidy[0] >= 2
