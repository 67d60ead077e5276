"""(GPU) ploidy 1 computed inside the ploidy-2 optimise job ("fuse_p1", optimize_kernel.h with_p1): every field of a call with the fusion equals the call
without it and the CPU oracle, bit for bit; where the fusion does not apply the call takes the ploidy-1 launches it always took.

The inputs are tiny random pileups (about 60 reads over 40 SNPs per contig, blocks of about a dozen SNPs) and three hand-made ones for the edges of the merged
statistics pass; the oracle runs once per input (module-scoped).  What each input must contain — a block that stops at ploidy 1, one that reaches ploidy >= 3,
a one-read block, a ploidy-2 partition of one read — is asserted from the oracle's result, so no test here passes vacuously."""
import numpy as np
import pytest

from floria_amd.pileup import Pileup
from tests.helpers import random_pileup

pytestmark = pytest.mark.gpu

EPS = 0.03125
FIELDS = ("best_ploidy", "ploidies_tried", "read_off", "read_id", "part")


class Case:
    """Contigs, blocks over them and the oracle's result for the batch (the oracle phases contig by contig: its results are joined block after block)."""

    def __init__(self, oracle, pileups, blocks, P=5, B=10, eps=EPS):
        self.pileups, self.P, self.B, self.eps = pileups, P, B, eps
        self.bc = [i for i, bl in enumerate(blocks) for _ in bl]
        self.bs = [s for bl in blocks for s, _ in bl]
        self.be = [e for bl in blocks for _, e in bl]
        rs = [oracle.phase_blocks(p, [s for s, _ in bl], [e for _, e in bl], oracle.make_params(eps, P, B), threads=4) for p, bl in zip(pileups, blocks)]
        self.best = np.concatenate([r.best_ploidy for r in rs])
        self.tried = np.concatenate([r.ploidies_tried for r in rs])
        self.mec = np.concatenate([r.mec for r in rs], axis=0)
        self.read_id = np.concatenate([r.read_id for r in rs])
        self.part = np.concatenate([r.part for r in rs])
        self.read_off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(r.read_off.astype(np.int64)) for r in rs]))]).astype(np.uint64)
        self.margin = min(r.min_prune_margin for r in rs)

    def check_oracle(self, r, what):
        assert np.array_equal(self.best, r.best_ploidy), (what, self.best, r.best_ploidy)
        assert np.array_equal(self.tried, r.ploidies_tried), (what, self.tried, r.ploidies_tried)
        assert np.array_equal(self.read_off, r.read_off) and np.array_equal(self.read_id, r.read_id), what
        assert np.array_equal(self.part, r.part), what
        assert np.array_equal(self.mec.view(np.uint64), r.mec.view(np.uint64)), (what, self.mec, r.mec)
        assert self.margin == r.min_prune_margin, (what, self.margin, r.min_prune_margin)

    def part_sizes(self, b):
        lo, hi = int(self.read_off[b]), int(self.read_off[b + 1])
        return np.bincount(self.part[lo:hi], minlength=int(self.best[b]))

    def n_jobs(self):
        return int(np.count_nonzero(np.diff(self.read_off.astype(np.int64))))


def same_bits(a, b, what):
    """every field of two results of the library with ==, the MEC values by their bit patterns (the zeros beyond ploidies_tried included)"""
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"
    assert a.mec.shape == b.mec.shape and np.array_equal(a.mec.view(np.uint64), b.mec.view(np.uint64)), f"{what}: mec"
    assert a.min_prune_margin == b.min_prune_margin, what


def windows(n_snps, length, step):
    return [(s, min(n_snps, s + length - 1)) for s in range(1, n_snps + 1, step)]


def small_contigs(seed, strains=(1, 2, 3, 4), errs=(0.002, 0.02, 0.02, 0.02), **kw):
    rng = np.random.default_rng(seed)
    return [random_pileup(rng, 60, 40, st, max_len=14, err=er, drop=0.05, **kw) for st, er in zip(strains, errs)]


@pytest.fixture(scope="module")
def small(oracle_mod):
    # four contigs of 1 / 2 / 3 / 4 strains (the one-strain contig with an error rate far below epsilon: its blocks stop at ploidy 1), four blocks each
    c = Case(oracle_mod, small_contigs(20261), [windows(40, 14, 10)] * 4)
    assert (c.best == 1).any() and (c.tried == 1).any(), "no block stops at ploidy 1"
    assert (c.tried >= 3).any(), "no block reaches ploidy 3"
    for b in np.nonzero(c.tried < c.P)[0]:
        assert (c.mec[b, c.tried[b]:] == 0).all()
    return c


@pytest.fixture(scope="module")
def many(oracle_mod):
    # the same kind of contigs under every SNP range of at most 32 SNPs: more than 3 x 1024 non-empty blocks, which is what three job groups ask for
    blocks = [(s, e) for s in range(1, 41) for e in range(s, min(40, s + 31) + 1)]
    c = Case(oracle_mod, small_contigs(20262), [blocks] * 4)
    assert c.n_jobs() >= 3 * 1024
    assert (c.tried == 1).any() and (c.tried >= 3).any()
    return c


@pytest.fixture
def knobs(gpu_ctx):
    """set_option for the test's duration: everything it touched is back at its default afterwards"""
    defaults = {"fuse_p1": -1, "groups": 0, "slots": 0, "speculate": -1, "arith": 0, "no_p1_shortcut": 0, "opt_global": 0, "opt_threads": 0}
    touched = set()

    def set_(**kv):
        for k, v in kv.items():
            assert k in defaults, k
            touched.add(k)
            gpu_ctx.set_option(k, v)
    yield set_
    for k in touched:
        gpu_ctx.set_option(k, defaults[k])


def run(ctx, lib, case, res, P=None):
    r = ctx.phase_blocks_batch(res, case.bc, case.bs, case.be, lib.make_params(case.eps, P or case.P, case.B))
    return r, ctx.timing()


def both(ctx, lib, case, knobs, what, groups=1):
    """the case with and without the fusion: equal to each other and to the oracle, and the fused call G launches short of the other"""
    res = ctx.upload_batch(case.pileups)
    try:
        knobs(fuse_p1=1)
        on, t_on = run(ctx, lib, case, res)
        knobs(fuse_p1=0)
        off, t_off = run(ctx, lib, case, res)
    finally:
        for r in res:
            r.free()
    same_bits(off, on, what)
    case.check_oracle(on, what + " (fused)")
    case.check_oracle(off, what + " (ploidy-1 launches)")
    assert t_on["streams"] == t_off["streams"] == groups, (what, t_on["streams"], t_off["streams"])
    assert t_off["optimize_launches"] == groups * case.P and t_on["optimize_launches"] == groups * (case.P - 1), (what, t_on, t_off)
    return on


def test_parity_on_small_random_pileups(gpu_ctx, hip_lib, small, knobs):
    knobs(speculate=0)
    both(gpu_ctx, hip_lib, small, knobs, "small pileups")
    knobs(fuse_p1=-1)          # the default is the fusion
    res = gpu_ctx.upload_batch(small.pileups)
    try:
        r, t = run(gpu_ctx, hip_lib, small, res)
    finally:
        for x in res:
            x.free()
    small.check_oracle(r, "default")
    assert t["optimize_launches"] == small.P - 1


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_job_groups(gpu_ctx, hip_lib, many, knobs, groups):
    knobs(speculate=0, groups=groups)
    both(gpu_ctx, hip_lib, many, knobs, f"{groups} job groups", groups)


def test_few_wave_slots_and_warm_pools(gpu_ctx, hip_lib, many, knobs):
    # 96 resident workgroups for more than 3 000 jobs of every launch; the second pair of calls finds the scratch pools of the first
    knobs(speculate=0, groups=2, slots=96)
    for rep in range(2):
        both(gpu_ctx, hip_lib, many, knobs, f"96 slots, call {rep}", 2)


def test_boundaries_of_the_merged_statistics(gpu_ctx, hip_lib, oracle_mod, knobs):
    q = np.full(10, 30)
    # contig 0: twenty reads of one haplotype over SNPs 1-10 and ONE read far away (SNPs 30-35): the block over it holds one read
    one_read = [(np.arange(1, 11), np.zeros(10, int), q)] * 20 + [(np.arange(30, 36), np.ones(6, int), q[:6])]
    # contig 1: twenty reads of one haplotype over SNPs 1-10, one read of the opposite one over SNPs 2-11: the ploidy-2 partition of that read holds it alone, SNP 11
    # is covered by that partition only and SNP 1 by the other only
    lone = [(np.arange(1, 11), np.zeros(10, int), q)] * 20 + [(np.arange(2, 12), np.ones(10, int), q)]
    c = Case(oracle_mod, [Pileup.from_reads(one_read), Pileup.from_reads(lone)], [[(1, 12), (28, 38)], [(1, 12)]])
    n = np.diff(c.read_off.astype(np.int64))
    assert list(n) == [20, 1, 21]
    assert c.best[2] == 2 and sorted(c.part_sizes(2)) == [1, 20], (c.best, c.part_sizes(2))
    knobs(speculate=0)
    both(gpu_ctx, hip_lib, c, knobs, "one-read block, one-read partition, position of one partition")


@pytest.mark.parametrize("knob, value, P", [("speculate", 1, 5), ("speculate", 2, 5), ("arith", 1, 5), ("fuse_p1", 1, 1), ("no_p1_shortcut", 1, 5)])
def test_fallbacks_take_the_ploidy_1_launches(gpu_ctx, hip_lib, oracle_mod, small, knobs, knob, value, P):
    # (epsilon is a multiple of 2^-10: the reference's running sums and the canonical form give the same bits, include/floria_hip.h)
    case = small if P == small.P else Case(oracle_mod, small.pileups, [windows(40, 14, 10)] * 4, P=P)
    res = gpu_ctx.upload_batch(case.pileups)
    try:
        knobs(speculate=0, fuse_p1=1)
        knobs(**{knob: value})
        r, t = run(gpu_ctx, hip_lib, case, res)
    finally:
        for x in res:
            x.free()
    case.check_oracle(r, f"{knob} = {value}, max_ploidy {P}")
    assert t["optimize_launches"] == t["streams"] * P, t


@pytest.mark.parametrize("variant", ["four_alleles", "q0", "opt_global", "opt_threads_128"])
def test_eligible_variants(gpu_ctx, hip_lib, oracle_mod, knobs, variant):
    kw = {"four_alleles": dict(alleles=4), "q0": dict(q0_frac=0.15)}.get(variant, {})
    c = Case(oracle_mod, small_contigs(20263, **kw), [windows(40, 14, 10)] * 4)
    assert (c.tried == 1).any() and (c.tried >= 3).any()
    knobs(speculate=0)
    if variant == "opt_global":
        knobs(opt_global=1)
    if variant == "opt_threads_128":
        knobs(opt_threads=128)
    both(gpu_ctx, hip_lib, c, knobs, variant)
