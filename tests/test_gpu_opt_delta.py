"""(GPU) the optimise kernel's delta pass ("opt_delta": in the canonical ploidy-specialised instances a read's distances are exact packed integers, and behind an
accepted round only the terms at the flipped (position, partition) code bytes are exchanged — optimize_kernel.h): a call with the option and a call without it give
the same best_ploidy, ploidies_tried, mec (bit patterns), read_off, read_id, part and min_prune_margin, and the oracle's; mec covers num_alleles and the stop rule,
and the rounds run (`iters`) are pinned by tests/opt_delta_model.py against the oracle on the CPU.

No case passes on a path it does not name: tests/opt_delta_model.py, the restatement of the rounds, runs every (block, ploidy) job of a case on the CPU, says which
pass every round takes and what it meets (a flip at a read's first / last cell, a read with a gap at the flipped position, code bytes that become / leave 0, two
exchanged cells in one read, a search that bisects, a read of more than 256 cells, more flips than the list holds, a rejected round behind an accepted one), and
predicts the library's counters optimize_delta_passes / optimize_delta_fallbacks, which the calls with one ploidy per stage must reproduce exactly.  The calls force
the 512-thread ploidy-specialised instances ("opt_threads" = 512), the ones that have the pass; one call on the 1024-thread instances and one on four alleles (the
generic instances) show that those take none and give the same results.  The 8-byte-cell form of the pass runs under "opt_packed" = 0."""
import numpy as np
import pytest

from floria_amd.pileup import Pileup
from tests import opt_delta_model as model
from tests.helpers import random_pileup

pytestmark = pytest.mark.gpu

EPS = 0.03125
FIELDS = ("best_ploidy", "ploidies_tried", "read_off", "read_id", "part")
DEFAULTS = {"opt_delta": 1, "opt_packed": 1, "opt_threads": 0, "speculate": -1, "groups": 0, "fuse_p1": -1}


@pytest.fixture
def knobs(gpu_ctx):
    touched = set()

    def set_(**kv):
        for k, v in kv.items():
            assert k in DEFAULTS, k
            touched.add(k)
            gpu_ctx.set_option(k, v)
    yield set_
    for k in touched:
        gpu_ctx.set_option(k, DEFAULTS[k])


class Case:
    """contigs, one block over each, the oracle's result, and the model's account of every (block, ploidy) job the reference runs"""

    def __init__(self, oracle, pileups, spans, P=5, alleles=2):
        self.pileups, self.P = pileups, P
        self.bc = list(range(len(pileups)))
        self.bs = [1] * len(pileups)
        self.be = list(spans)
        self.oracle = [oracle.phase_blocks(p, [1], [e], oracle.make_params(EPS, P, 10), threads=4) for p, e in zip(pileups, spans)]
        self.passes = self.fallbacks = 0
        self.met = set()
        if alleles != 2:          # (the ploidy-specialised instances are biallelic: no delta pass, nothing to predict)
            return
        w24 = oracle.weight_q24()
        for p, e, o in zip(pileups, spans, self.oracle):
            for ploidy in range(2, int(o.ploidies_tried[0]) + 1):
                rid, pb, po, _, _, iters = oracle.one_ploidy(p, 1, e, ploidy, EPS)
                part, it, rounds = model.run(p, rid, pb, ploidy, EPS, w24)
                assert np.array_equal(part, po) and it == iters
                for x, r in enumerate(rounds):
                    self.passes += r["pass"] == "delta"
                    self.fallbacks += r["pass"] == "interval"
                    if r["pass"] == "delta":
                        self.met |= r["met"]
                    if r["pass"] == "interval" and len(r["flips"]) > model.FLIP_CAP:
                        self.met.add("overflow")
                    if not r["accepted"] and x > 0 and rounds[x - 1]["pass"] == "delta":
                        self.met.add("rejected_after_delta")

    def check(self, r, what):
        ro = r.read_off.astype(np.int64)
        for b, o in enumerate(self.oracle):
            assert int(o.best_ploidy[0]) == int(r.best_ploidy[b]) and int(o.ploidies_tried[0]) == int(r.ploidies_tried[b]), (what, b)
            assert np.array_equal(o.mec.view(np.uint64), r.mec[b:b + 1].view(np.uint64)), (what, b, o.mec, r.mec[b])
            lo, hi = int(ro[b]), int(ro[b + 1])
            assert np.array_equal(o.read_id, r.read_id[lo:hi]) and np.array_equal(o.part, r.part[lo:hi]), (what, b)
        assert min(o.min_prune_margin for o in self.oracle) == r.min_prune_margin, what


def same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"
    assert a.mec.shape == b.mec.shape and np.array_equal(a.mec.view(np.uint64), b.mec.view(np.uint64)), f"{what}: mec"
    assert a.min_prune_margin == b.min_prune_margin, f"{what}: min_prune_margin"


def on_and_off(ctx, lib, case, knobs, what, exact=True, threads=512, delta=True, **more):
    """the case with opt_delta = 1 and = 0: equal to each other and to the oracle, and the counters what the model predicts (exact = False: a speculative stage runs
    and drops jobs of its own, so only `at least one delta pass` holds; delta = False: the call takes instances that have no delta pass, both counters stay 0)"""
    res = ctx.upload_batch(case.pileups)
    out = []
    try:
        knobs(opt_threads=threads, **more)
        for on in (1, 0):
            knobs(opt_delta=on)
            out.append(ctx.phase_blocks_batch(res, case.bc, case.bs, case.be, lib.make_params(EPS, case.P, 10)))
            t = ctx.timing()
            print(what, "opt_delta", on, "passes", t["optimize_delta_passes"], "fallbacks", t["optimize_delta_fallbacks"], "predicted", case.passes, case.fallbacks)
            if not on or not delta:
                assert t["optimize_delta_passes"] == 0 and t["optimize_delta_fallbacks"] == 0, what
            elif exact:
                assert (t["optimize_delta_passes"], t["optimize_delta_fallbacks"]) == (case.passes, case.fallbacks), what
            else:
                assert t["optimize_delta_passes"] >= 1, what
    finally:
        for x in res:
            x.free()
    same_bits(out[0], out[1], f"{what}: opt_delta = 0 against the default")
    for r in out:
        case.check(r, what)


def sparse_and_dense(seed, n=12):
    """blocks of 8-64 reads over 8-48 SNPs, 2-4 strains, reads of up to 48 cells that skip none, a tenth or four tenths of their positions"""
    rng = np.random.default_rng(seed)
    piles, spans = [], []
    for _ in range(n):
        n_snps = int(rng.integers(8, 49))
        piles.append(random_pileup(rng, int(rng.integers(8, 65)), n_snps, int(rng.integers(2, 5)), max_len=int(rng.integers(12, 49)), err=0.12, drop=float(rng.choice([0.0, 0.1, 0.4]))))
        spans.append(n_snps)
    return piles, spans


@pytest.fixture(scope="module")
def small(oracle_mod):
    (pa, sa), (pb, sb) = sparse_and_dense(9301), sparse_and_dense(9303)          # (between them the two seeds meet every case of SMALL_MEETS)
    return Case(oracle_mod, pa + pb, sa + sb)


SMALL_MEETS = {"first", "last", "gap", "to0", "from0", "two_same", "two_diff", "rejected_after_delta"}


@pytest.mark.parametrize("fuse_p1", [0, 1])
@pytest.mark.parametrize("packed", [1, 0])
def test_small_blocks_packed_and_wide_cells_with_and_without_fused_ploidy_1(gpu_ctx, hip_lib, knobs, small, packed, fuse_p1):
    # (opt_packed = 0: the same jobs on the 8-byte cells, whose delta pass searches cell_snp)
    assert small.passes >= 5 and small.fallbacks >= 1 and SMALL_MEETS <= small.met, (small.passes, small.fallbacks, SMALL_MEETS - small.met)
    lens = [int(x) % 4 for p in small.pileups for x in p.read_off[:-1]]
    assert set(lens) == {0, 1, 2, 3}          # (first cells at every offset of a 16-byte piece)
    on_and_off(gpu_ctx, hip_lib, small, knobs, f"small blocks, opt_packed {packed}, fuse_p1 {fuse_p1}", speculate=0, opt_packed=packed, fuse_p1=fuse_p1)


def test_a_speculative_stage(gpu_ctx, hip_lib, knobs, small):
    on_and_off(gpu_ctx, hip_lib, small, knobs, "small blocks, speculate 1", exact=False, speculate=1)


def test_the_1024_thread_instances_take_no_delta_pass(gpu_ctx, hip_lib, knobs, small):
    # (they keep the f64 slots and the interval pass: optimize_kernel.h, DELTA)
    on_and_off(gpu_ctx, hip_lib, small, knobs, "small blocks, opt_threads 1024", threads=1024, delta=False, speculate=0)


def long_reads(seed, n_snps=330):
    """40 reads of 100-330 cells (one in twenty positions skipped) in three strains: reads of more than 256 cells, searches that bisect, and rounds that move a read
    into a partition with nothing yet at its positions — more than 64 code bytes flip at once"""
    rng = np.random.default_rng(seed)
    hap = rng.integers(0, 2, size=(3, n_snps))
    reads = []
    for _ in range(40):
        L = int(rng.integers(100, n_snps + 1))
        s = int(rng.integers(1, n_snps - L + 2))
        snps = np.arange(s, s + L)
        keep = rng.random(L) >= 0.05
        keep[0] = True
        snps = snps[keep]
        al = hap[int(rng.integers(0, 3)), snps - 1].copy()
        flip = rng.random(len(snps)) < 0.15
        al[flip] ^= 1
        reads.append((snps, al, rng.integers(5, 41, size=len(snps))))
    return [Pileup.from_reads(reads)], [n_snps]


def test_long_reads_and_more_flips_than_the_list_holds(gpu_ctx, hip_lib, oracle_mod, knobs):
    c = Case(oracle_mod, *long_reads(9312))
    assert c.passes >= 1 and {"long", "bisect", "overflow"} <= c.met, (c.passes, c.fallbacks, c.met)
    on_and_off(gpu_ctx, hip_lib, c, knobs, "long reads", speculate=0)


def test_four_alleles_take_no_delta_pass(gpu_ctx, hip_lib, oracle_mod, knobs):
    rng = np.random.default_rng(9320)
    piles = [random_pileup(rng, 50, 40, st, max_len=30, alleles=4, err=0.12) for st in (2, 3)]
    assert set(int(x) for p in piles for x in p.allele) == {0, 1, 2, 3}
    c = Case(oracle_mod, piles, [40, 40], alleles=4)
    on_and_off(gpu_ctx, hip_lib, c, knobs, "alleles 0-3", speculate=0)
