"""Inputs for the kernels that run AFTER S1 (hap graph, haploset statistics, HAPQ, S2), built so that each lands on a code path that takes over once an
input exceeds a fixed capacity.  tests/test_after_s1_cases_cpu.py proves from the oracle alone that every case is in the regime it is meant for;
tests/test_gpu_after_s1_paths.py compares the device with the oracle on the same cases and repeats the regime guards on what the device returns.

Everything is deterministic (np.random.default_rng with fixed seeds) and built on tests.helpers.random_pileup and Pileup.from_reads.

The capacities, named once:
  GRAPH_HIST_LDS_BYTES  floria_hip_hap_graph (floria_amd/csrc/floria_hip.hip) keeps the histogram of graph_kernel in LDS while range_max * pmax * A * 8 bytes fit in it
  GRAPH_SORT_CAP        floria_amd/csrc/graph_kernel.h: the allele counts of one node are sorted in LDS while range * A fits in it
  TRIP                  floria_amd/csrc/stats_kernel.h, floria_amd/csrc/hapq_kernel.h: the per-position loops stride by one workgroup of 256 threads
  PAIR_TRIP             floria_amd/csrc/hapq_kernel.h pair_kernel: one wavefront of 64 lanes over the intersection of two spans
  CHAIN_FAST_CELLS / CHAIN_FAST_CANDS   floria_amd/csrc/reassign_kernel.h reassign_chain_kernel: register fast path for L <= 256 cells and nc <= 64 candidate groups;
                        reassign_kernel<A, true> folds the candidates 64 per trip
  DENSE_RULE            floria_hip_reassign_batch: a contig takes the chain kernel when (reads with a choice) * 8 >= reads visited
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from floria_amd.pileup import Pileup
from tests.helpers import random_pileup

GRAPH_HIST_LDS_BYTES = 40 * 1024
GRAPH_SORT_CAP = 2048
TRIP = 256
PAIR_TRIP = 64
CHAIN_FAST_CELLS = 256
CHAIN_FAST_CANDS = 64
DENSE_RULE = 8
EPS = 0.03125


# ---- small tools on pileups ------------------------------------------------------------------------------------------------------------------------
def reads_of(p, shift=0):
    return [(p.read(r)[0].astype(np.int64) + shift, p.read(r)[1], p.read(r)[2]) for r in range(p.n_reads)]


def merged(*parts):
    """One pileup from the reads of several, each given as (pileup, SNP shift) or (pileup, SNP shift, keep mask)"""
    reads = []
    for part in parts:
        p, shift = part[0], part[1]
        rs = reads_of(p, shift)
        if len(part) > 2:
            rs = [r for r, k in zip(rs, part[2]) if k]
        reads += rs
    return Pileup.from_reads(reads)


def n_snps_of(p):
    return int(p.last.max())


def n_alleles_of(p):
    return 4 if int(p.allele.max()) > 1 else 2


# ---- 1. hap graph ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class GraphCase:
    name: str
    pileups: list                 # one per contig
    blk_contig: np.ndarray
    blk_start: np.ndarray
    blk_end: np.ndarray
    hist_in_lds: bool             # the regime the case is meant for
    sort_in_lds: bool
    max_ploidy: int = 4
    beam: int = 6
    min_best_ploidy: int = 0      # max(best_ploidy) the case needs at least ...
    max_best_ploidy: int = 99     # ... and at most
    eps: float = EPS
    expect: dict = field(default_factory=dict)      # bookkeeping the case is about: block index -> best_ploidy property

    def blocks_of(self, ci):
        m = self.blk_contig == ci
        return self.blk_start[m], self.blk_end[m], np.nonzero(m)[0]


def graph_regime(case, best_ploidy):
    """(histogram bytes, sort cells) as floria_hip_hap_graph computes them: over the NON-EMPTY blocks of the call"""
    bp = np.asarray(best_ploidy)
    ne = bp > 0
    rng_len = (case.blk_end.astype(np.int64) - case.blk_start.astype(np.int64) + 1)
    range_max = int(rng_len[ne].max()) if ne.any() else 1
    A = max(n_alleles_of(p) for p in case.pileups)
    return range_max * int(bp.max()) * A * 8, range_max * A


def assert_graph_regime(case, best_ploidy):
    hist_bytes, sort_cells = graph_regime(case, best_ploidy)
    pm = int(np.max(best_ploidy))
    assert case.min_best_ploidy <= pm <= case.max_best_ploidy, (case.name, "max best_ploidy", pm)
    assert (hist_bytes <= GRAPH_HIST_LDS_BYTES) == case.hist_in_lds, (case.name, "histogram bytes", hist_bytes)
    assert (sort_cells <= GRAPH_SORT_CAP) == case.sort_in_lds, (case.name, "sort cells", sort_cells)
    for b, want in case.expect.items():
        got = int(best_ploidy[b])
        assert (got == 0) if want == "empty" else (got == 1) if want == "one" else (got >= 2), (case.name, "block", b, "best_ploidy", got, want)


def _one_contig(name, pile, blocks, **kw):
    s = np.array([b[0] for b in blocks], np.uint32); e = np.array([b[1] for b in blocks], np.uint32)
    return GraphCase(name, [pile], np.zeros(len(blocks), np.uint32), s, e, **kw)


def _graph_both_pools():
    # three blocks of 1100 SNPs over 1800: 1100 * 3 * 2 * 8 = 52 800 B > 40 KiB, 2200 cells > 2048
    pile = random_pileup(np.random.default_rng(4101), 260, 1800, 3, max_len=260, err=0.01, drop=0.05)
    return _one_contig("biallelic_both_pools", pile, [(1, 1100), (351, 1450), (701, 1800)], hist_in_lds=False, sort_in_lds=False, min_best_ploidy=3)


@lru_cache(maxsize=None)
def _boundary_pileup():
    return random_pileup(np.random.default_rng(4102), 220, 1540, 2, max_len=260, err=0.01, drop=0.05)


def _graph_sort_boundary(n):
    # ranges of exactly n SNPs: n * 2 = 2048 is the last LDS sort, 2050 the first sort in the pool.  Planted ploidy 2: 1025 * 2 * 2 * 8 = 32 800 B stays in LDS
    return _one_contig(f"biallelic_sort_boundary_{n}", _boundary_pileup(), [(1, n), (501, 500 + n)], hist_in_lds=True, sort_in_lds=n * 2 <= GRAPH_SORT_CAP,
                       min_best_ploidy=2, max_best_ploidy=2, max_ploidy=4)


def _graph_four_alleles():
    # ranges of 600 SNPs with four alleles: 2400 cells > 2048; 600 * 3 * 4 * 8 = 57 600 B > 40 KiB
    pile = random_pileup(np.random.default_rng(4103), 220, 1000, 3, max_len=200, alleles=4, err=0.01, drop=0.05)
    return _one_contig("four_alleles_both_pools", pile, [(1, 600), (201, 800), (401, 1000)], hist_in_lds=False, sort_in_lds=False, min_best_ploidy=3)


def _graph_hist_pool_lds_sort():
    # range 700, biallelic: 1400 cells sort in LDS; 700 * 4 * 2 * 8 = 44 800 B > 40 KiB once some block has best_ploidy >= 4
    pile = random_pileup(np.random.default_rng(4104), 300, 1100, 4, max_len=220, err=0.005, drop=0.05)
    return _one_contig("hist_pool_lds_sort", pile, [(1, 700), (201, 900), (401, 1100)], hist_in_lds=False, sort_in_lds=True, min_best_ploidy=4, max_ploidy=5, beam=8)


def _graph_bookkeeping():
    # contig 0: SNPs 1..1800 three planted haplotypes with a stretch [1150, 1180] that no read touches, SNPs 1801..2300 ONE haplotype without errors.
    #   block 0 (1, 1100)       pool-sized
    #   block 1 (1150, 1180)    empty: best_ploidy 0, the next block's pred skips it
    #   block 2 (601, 1700)     pool-sized, shares the reads of 601..1100 with block 0
    #   block 3 (1401, 2000)    mixed
    #   block 4 (1851, 2300)    one node (p2 == 1): every read it shares with block 3 counts as unambiguous
    # contig 1: two more pool-sized blocks, so that the pool slices are addressed by block index across contigs
    a = random_pileup(np.random.default_rng(4105), 260, 1800, 3, max_len=260, err=0.01, drop=0.05)
    keep = ~((a.last >= 1150) & (a.first <= 1180))
    b = random_pileup(np.random.default_rng(4106), 60, 500, 1, max_len=120, err=0.0, drop=0.05)
    c0 = merged((a, 0, keep), (b, 1800))
    c1 = random_pileup(np.random.default_rng(4107), 200, 1400, 3, max_len=260, err=0.01, drop=0.05)
    blocks = [(0, 1, 1100), (0, 1150, 1180), (0, 601, 1700), (0, 1401, 2000), (0, 1851, 2300), (1, 1, 1050), (1, 351, 1400)]
    return GraphCase("bookkeeping_two_contigs", [c0, c1], np.array([x[0] for x in blocks], np.uint32), np.array([x[1] for x in blocks], np.uint32),
                     np.array([x[2] for x in blocks], np.uint32), hist_in_lds=False, sort_in_lds=False, min_best_ploidy=3,
                     expect={0: "many", 1: "empty", 2: "many", 4: "one", 5: "many", 6: "many"})


_GRAPH = {"biallelic_both_pools": _graph_both_pools, "biallelic_sort_boundary_1024": lambda: _graph_sort_boundary(1024),
          "biallelic_sort_boundary_1025": lambda: _graph_sort_boundary(1025), "four_alleles_both_pools": _graph_four_alleles,
          "hist_pool_lds_sort": _graph_hist_pool_lds_sort, "bookkeeping_two_contigs": _graph_bookkeeping}
GRAPH_CASES = tuple(_GRAPH)


@lru_cache(maxsize=None)
def graph_case(name):
    return _GRAPH[name]()


def oracle_graph(oracle_mod, case):
    """per contig: (oracle S1 result, node_cov, edge_w, block indices of the contig)"""
    out = []
    for ci, pile in enumerate(case.pileups):
        s, e, idx = case.blocks_of(ci)
        ro = oracle_mod.phase_blocks(pile, s, e, oracle_mod.make_params(case.eps, case.max_ploidy, case.beam), threads=8)
        cov, ew = oracle_mod.hap_graph(pile, s, e, ro)
        out.append((ro, cov, ew, idx))
    return out


# ---- 2. haploset statistics and HAPQ ---------------------------------------------------------------------------------------------------------------
RANGE_LENGTHS = (1, 255, 256, 257, 511, 513, 1400)
PAIR_KINDS = ("disjoint", "touch", "overlap63", "overlap64", "overlap65", "contains")
STATS_SNPS = 1500
PAIR_REGION = 250             # every crafted pair lives in a region of its own, so that in the pairs-only list a group has exactly one partner


@dataclass
class StatsCase:
    name: str
    pileup: Pileup
    snp_pos: np.ndarray
    block_length: int
    groups: list
    ranges: list
    n_length_groups: int          # groups [0, n_length_groups): the range-length groups and the three degenerate ones; the rest: crafted pairs
    pair_groups: dict             # kind -> (index of group i, index of group j)

    def pairs_only(self):
        k = self.n_length_groups
        return self.groups[k:], self.ranges[k:]


def spans_of(pile, groups):
    """(lo, len) of every group's reads, as floria_hip_hapq_batch computes them: len 0 for an empty group"""
    lo = np.zeros(len(groups), np.int64); ln = np.zeros(len(groups), np.int64)
    for k, g in enumerate(groups):
        if len(g):
            lo[k] = int(pile.first[g].min()); ln[k] = int(pile.last[g].max()) - lo[k] + 1
    return lo, ln


def selected_pairs(ranges):
    """find_overlapping_blocks (part_block_manip.rs:453-513) as oracle.hapq restates it: half-open overlap of the SNP ranges, overlap_percent > 0.05;
    u32 arithmetic as there.  The oracle has no entry point that returns the pairs, so this is a copy of the loop in oracle/floria_oracle.cpp (hapq) and
    has to be kept in step with it by hand"""
    out = []
    u = lambda x: int(x) & 0xffffffff
    for i, (x1, x2) in enumerate(ranges):
        for j, (y1, y2) in enumerate(ranges):
            if j == i or not (y1 < x2 and y2 > x1):
                continue
            ol = min(1.0, min(u(x2 - y1 + 1), u(y2 - x1 + 1)) / u(x2 - x1 + 1))
            if ol > 0.05:
                out.append((i, j))
    return out


def pair_kind(lo, ln, i, j):
    """how the spans of two groups lie to each other, as pair_kernel sees them: kind and the offset of the intersection inside each span"""
    if ln[i] == 0 or ln[j] == 0:
        return "empty", 0, 0
    a = max(lo[i], lo[j]); b = min(lo[i] + ln[i], lo[j] + ln[j])          # [a, b)
    n = int(b - a)
    oi, oj = int(a - lo[i]), int(a - lo[j])
    if n <= 0:
        return "disjoint", oi, oj
    if n == ln[i] or n == ln[j]:
        return "contains", oi, oj
    if n == 1:
        return "touch", oi, oj
    return f"overlap{n}", oi, oj


def count_pair_kinds(pile, groups, ranges):
    """kind -> number of selected pairs of that kind whose intersection starts at a non-zero offset in at least one span"""
    lo, ln = spans_of(pile, groups)
    cnt = {}
    for i, j in selected_pairs(ranges):
        kind, oi, oj = pair_kind(lo, ln, i, j)
        if kind.startswith("overlap") and max(oi, oj) == 0:
            continue
        cnt[kind] = cnt.get(kind, 0) + 1
    return cnt


def _subset(rng, ids, frac, must=()):
    pick = ids[rng.random(len(ids)) < frac]
    return np.unique(np.concatenate([pick, np.asarray(must, np.int64)])).astype(np.uint32)


def _crafted_pair(rng, pile, kind, r0, r1):
    """two groups of reads inside SNPs [r0, r1] whose spans lie to each other as `kind` says; both get the range (r0, r1), so find_overlapping_blocks selects
    the pair whatever the spans do"""
    ids = np.arange(pile.n_reads)
    first, last = pile.first.astype(np.int64), pile.last.astype(np.int64)
    inside = (first >= r0) & (last <= r1)
    mid = (r0 + r1) // 2
    if kind == "contains":
        outer = ids[inside]
        lo_o, hi_o = first[outer].min(), last[outer].max()
        inner = ids[inside & (first >= lo_o + 20) & (last <= hi_o - 20)]
        assert len(inner) >= 3
        return _subset(rng, outer, 0.7, must=(outer[np.argmin(first[outer])], outer[np.argmax(last[outer])])), _subset(rng, inner, 0.7, must=inner[:1])
    n = {"disjoint": -10, "touch": 1}.get(kind) or int(kind[len("overlap"):])
    # group i ends at last[ra] = m, group j starts at first[rb] = m - n + 1: n common positions (n <= 0: a gap)
    for ra in ids[inside & (last >= mid - 30) & (last <= mid + 30)]:
        m = last[ra]
        for rb in ids[inside & (first == m - n + 1)]:
            gi = ids[inside & (last <= m)]
            gj = ids[inside & (first >= m - n + 1)]
            if rb == ra or len(gi) < 4 or len(gj) < 4:
                continue
            return _subset(rng, gi, 0.7, must=(ra,)), _subset(rng, gj, 0.7, must=(rb,))
    raise AssertionError(f"no reads for a pair of kind {kind} in [{r0}, {r1}]")


def _stats_case(name, alleles):
    rng = np.random.default_rng(4200 + alleles)
    if alleles == 4:        # equal qualities and q = 0 cells: ties everywhere, and sites with all four alleles (the 0,2,1,3 order)
        pile = random_pileup(rng, 480, STATS_SNPS, 3, max_len=80, alleles=4, qlo=20, qhi=20, err=0.3, q0_frac=0.1)
    else:
        pile = random_pileup(rng, 480, STATS_SNPS, 3, max_len=80, alleles=2, err=0.1)
    S = n_snps_of(pile)
    ids = np.arange(pile.n_reads)
    groups, ranges = [], []
    for k, n in enumerate(RANGE_LENGTHS):
        lo = 1 + (37 * (k + 1)) % (S - n)
        hi = lo + n - 1
        m = (pile.first <= hi) & (pile.last >= lo)
        groups.append(_subset(rng, ids[m], 0.85)); ranges.append((lo, hi))
    groups.append(np.zeros(0, np.uint32)); ranges.append((3, 900))                                   # an empty group: err = 0 / 0
    groups.append(_subset(rng, ids[pile.last < 600], 0.2)); ranges.append((700, 1300))                # reads wholly outside the range
    groups.append(_subset(rng, ids[(pile.first <= 500) & (pile.last >= 400)], 0.5)); ranges.append((500, 400))      # hi < lo
    n_len = len(groups)
    pair_groups = {}
    for k, kind in enumerate(PAIR_KINDS):
        r0, r1 = 1 + k * PAIR_REGION, (k + 1) * PAIR_REGION
        gi, gj = _crafted_pair(rng, pile, kind, r0, r1)
        pair_groups[kind] = (len(groups), len(groups) + 1)
        groups += [gi, gj]; ranges += [(r0, r1), (r0, r1)]
    snp_pos = np.cumsum(rng.integers(50, 400, size=S)).astype(np.uint64)
    # block_length well below the genome span of a pair region (about 56 kb): 40 * ln(base_range / block_length + 1) is then just under the cap of 60 for
    # the crafted pairs, so their HAPQ moves with the same / diff counts of pair_kernel
    return StatsCase(name, pile, snp_pos, 17000, groups, ranges, n_len, pair_groups)


STATS_CASES = ("two_alleles", "four_alleles")


@lru_cache(maxsize=None)
def stats_case(name):
    return _stats_case(name, 2 if name == "two_alleles" else 4)


# ---- 3. S2 -----------------------------------------------------------------------------------------------------------------------------------------
CAND_CYCLE = (1, 2, 63, 64, 65, 127, 128, 129, 140)
LONG_LENGTHS = (255, 256, 257, 300, 650)


@dataclass
class S2Case:
    name: str
    pileup: Pileup
    groups: list
    ranges: list
    dense: object                 # True: auto routing takes the chain kernel; False: the parallel one; None: not asserted
    orders: list = field(default_factory=list)      # visiting orders beyond ascending


def candidate_counts(case):
    """number of groups every read sits in, recomputed from the group lists (a group is a set)"""
    n = np.zeros(case.pileup.n_reads, np.int64)
    for g in case.groups:
        n[np.unique(g)] += 1
    return n


def read_lengths(pile):
    return np.diff(pile.read_off.astype(np.int64))


def is_dense(case, order=None):
    """the host's routing rule: reads with a choice * 8 >= reads visited (and at least one read has a choice)"""
    nc = candidate_counts(case)
    visited = nc if order is None else nc[np.asarray(order)]
    nm = int((visited > 1).sum())
    return nm > 0 and nm * DENSE_RULE >= len(visited)


def _random_membership(rng, n_reads, n_groups, k_of_read):
    member = [[] for _ in range(n_groups)]
    for r in range(n_reads):
        for g in rng.choice(n_groups, size=int(k_of_read[r]), replace=False):
            member[int(g)].append(r)
    return [np.array(sorted(m), np.uint32) for m in member]


def _orders(rng, case, n=1):
    members = np.unique(np.concatenate([g for g in case.groups if len(g)]))
    return [rng.permutation(members).astype(np.uint32) for _ in range(n)]


def _s2_many_candidates():
    rng = np.random.default_rng(4301)
    a = random_pileup(rng, 75, 40, 3, max_len=25, qlo=20, qhi=20, err=0.1)         # equal qualities: (diff + 1, id, same) ties on diff
    b = random_pileup(rng, 75, 40, 3, max_len=25, err=0.1)
    pile = merged((a, 0), (b, 0))
    S = n_snps_of(pile)
    k = np.array([CAND_CYCLE[i % len(CAND_CYCLE)] for i in range(pile.n_reads)])
    case = S2Case("many_candidates", pile, _random_membership(rng, pile.n_reads, 140, k), [(1, S)] * 140, True)
    case.orders = _orders(rng, case, 2)
    return case


def _long_reads(rng, n_reads, n_snps, alleles, lengths):
    """reads of exactly the given cell counts (contiguous SNPs), then random ones"""
    hap = rng.integers(0, alleles, size=(3, n_snps))
    reads = []
    for i in range(n_reads):
        L = lengths[i] if i < len(lengths) else int(rng.integers(20, 280))
        s = int(rng.integers(1, n_snps - L + 2))
        snps = np.arange(s, s + L)
        al = hap[int(rng.integers(0, 3)), snps - 1].copy()
        flip = rng.random(L) < 0.08
        al[flip] = rng.integers(0, alleles, size=int(flip.sum()))
        reads.append((snps, al, rng.integers(5, 41, size=L)))
    return Pileup.from_reads(reads)


def _s2_long_reads(alleles):
    rng = np.random.default_rng(4310 + alleles)
    pile = _long_reads(rng, 60, 700, alleles, LONG_LENGTHS)
    S = n_snps_of(pile)
    k = rng.integers(2, 4, size=pile.n_reads)                                      # every read sits in 2-3 of the 6 groups
    case = S2Case(f"long_reads_{alleles}_alleles", pile, _random_membership(rng, pile.n_reads, 6, k), [(1, S)] * 6, True)
    case.orders = _orders(rng, case, 1)
    return case


def _s2_long_and_many():
    # both limits of the chain kernel's fast path in one read: 257 cells and 65 candidate groups
    rng = np.random.default_rng(4320)
    pile = _long_reads(rng, 40, 400, 2, (257, 256, 300))
    S = n_snps_of(pile)
    L = read_lengths(pile)
    k = rng.integers(2, 6, size=pile.n_reads)
    k[int(np.nonzero(L == 257)[0][0])] = 65
    k[int(np.nonzero(L == 256)[0][0])] = 64
    k[int(np.nonzero(L == 300)[0][0])] = 70
    case = S2Case("long_and_many", pile, _random_membership(rng, pile.n_reads, 70, k), [(1, S)] * 70, True)
    case.orders = _orders(rng, case, 1)
    return case


def _strain_groups(rng, cfg, idx, scale, n_groups, extra_frac):
    """haplogroups as they come out of stitching (test_reassign_sparse_choices_parallel_kernel): every read in the group of its strain, a fraction of the
    reads in one or two more"""
    from floria_amd import synth
    c = synth.make_config_contig(cfg, idx, scale, keep_truth=True)
    p = c.pileup
    groups = [np.nonzero(c.strain % n_groups == k)[0].astype(np.uint32) for k in range(n_groups)]
    if extra_frac:
        for r in rng.choice(p.n_reads, size=max(4, int(p.n_reads * extra_frac)), replace=False):
            for k in rng.choice(n_groups, size=int(rng.integers(1, 3)), replace=False):
                if r not in groups[k]:
                    groups[k] = np.sort(np.append(groups[k], np.uint32(r)))
    return p, groups, [(1, n_snps_of(p))] * n_groups


def _s2_sparse():
    rng = np.random.default_rng(21)
    p, groups, ranges = _strain_groups(rng, 4, 6, 1.0, 4, 1 / 40)
    case = S2Case("sparse_choices", p, groups, ranges, False)
    case.orders = [rng.permutation(p.n_reads).astype(np.uint32)]
    return case


def _s2_dense():
    # the haplogroups of overlapping blocks, unstitched (test_reassign_parity): most reads sit in two or three; S1 by the oracle, so the case needs no device
    from floria_amd import synth
    from oracle import oracle
    oracle.build()
    c = synth.make_config_contig(4, 2, 0.5)
    s, e = oracle.block_ranges(c.snp_pos, 10000)
    r = oracle.phase_blocks(c.pileup, s, e, oracle.make_params(EPS), threads=8)
    groups, ranges = [], []
    for b in range(r.n_blocks):
        for part in r.partitions(b):
            if len(part):
                groups.append(part); ranges.append((int(s[b]), int(e[b])))
    case = S2Case("dense_choices", c.pileup, groups, ranges, True)
    case.orders = _orders(np.random.default_rng(22), case, 1)
    return case


def _s2_no_choice():
    p, groups, ranges = _strain_groups(np.random.default_rng(23), 4, 9, 0.5, 3, 0)
    return S2Case("no_choice", p, groups, ranges, False)


def _s2_no_groups():
    return S2Case("no_groups", random_pileup(np.random.default_rng(4330), 40, 30, 2), [], [], False)


_S2 = {"many_candidates": _s2_many_candidates, "long_reads_2_alleles": lambda: _s2_long_reads(2), "long_reads_4_alleles": lambda: _s2_long_reads(4),
       "long_and_many": _s2_long_and_many, "sparse_choices": _s2_sparse, "dense_choices": _s2_dense, "no_choice": _s2_no_choice, "no_groups": _s2_no_groups}
S2_CASES = tuple(_S2)
MIXED_BATCH = ("dense_choices", "sparse_choices", "no_choice", "no_groups", "many_candidates")


@lru_cache(maxsize=None)
def s2_case(name):
    return _S2[name]()


def assert_s2_regime(case):
    nc = candidate_counts(case)
    L = read_lengths(case.pileup)
    if case.name in ("many_candidates",):
        for k in (64, 65, 128, 129):
            assert (nc == k).any(), (case.name, "no read with", k, "candidates")
        assert set(CAND_CYCLE) <= set(nc.tolist())
    if case.name.startswith("long_reads"):
        for n in LONG_LENGTHS:
            assert (L == n).any(), (case.name, "no read of", n, "cells")
        assert (nc[L > CHAIN_FAST_CELLS] > 1).all() and (L > CHAIN_FAST_CELLS).sum() >= 3
        assert nc.min() >= 2 and nc.max() <= 3
    if case.name == "long_and_many":
        assert ((L == 257) & (nc == 65)).any() and ((L == 256) & (nc == 64)).any() and ((L > CHAIN_FAST_CELLS) & (nc > CHAIN_FAST_CANDS)).sum() >= 2
    if case.name == "no_choice":
        assert nc.max() == 1
    if case.dense is not None and len(case.groups):
        for order in [None] + list(case.orders):
            assert is_dense(case, order) == case.dense, (case.name, "density")
