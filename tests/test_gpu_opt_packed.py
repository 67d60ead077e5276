"""(GPU) the optimise kernel's 4-byte cell stream ("opt_packed": optimize_kernel<.., PK = true> reads ContigDev::cell_pk with 16-byte loads, eight lanes per
read, weights from a table in LDS): a call with the option and a call without it give the same best_ploidy, ploidies_tried, mec (bit patterns), read_off,
read_id, part and min_prune_margin on every block, and the oracle's on the blocks it phased.  (The zigzag visiting order that was measured together with
the packed stream did not pay and is not in the library, profiles/opt_packed.md; with it, these cases ran under all four combinations of the two options.)

Small shapes at which the packed stream can go wrong: read lengths around the 4-cell piece, the 32 / 64 / 128-cell trips and beyond; first cells at every offset
mod 4, the contig's last read ending at the very end of the array; blocks of 1 .. 33 reads (the eight-lane groups); the quality bytes at the ends
of the weight table; SNP indices past 65 536; every ploidy with and without the fused ploidy 1; several optimise rounds and a rejected one; and the calls that
must stay on the 8-byte cells (four alleles, a device-assembled contig in the batch).  Every call forces the 512-thread ploidy-specialised instances
("opt_threads" = 512), which are the ones that have a packed form, and the timing's optimize_packed_launches says which stream a call took, so that no case
passes on the path it does not name."""
import numpy as np
import pytest

from floria_amd.pileup import Pileup
from tests.helpers import random_pileup

pytestmark = pytest.mark.gpu

EPS = 0.03125
FIELDS = ("best_ploidy", "ploidies_tried", "read_off", "read_id", "part")
COMBOS = [1, 0]          # opt_packed; the first is the default
DEFAULTS = {"opt_packed": 1, "opt_threads": 0, "speculate": -1, "groups": 0, "fuse_p1": -1, "slots": 0}


class Case:
    """contigs, blocks over them, and the oracle's result for the contigs in `check` (all of them by default), block after block"""

    def __init__(self, oracle, pileups, blocks, P=5, B=10, eps=EPS, check=None):
        self.pileups, self.P, self.B, self.eps = pileups, P, B, eps
        self.bc = [i for i, bl in enumerate(blocks) for _ in bl]
        self.bs = [s for bl in blocks for s, _ in bl]
        self.be = [e for bl in blocks for _, e in bl]
        self.check = list(range(len(pileups))) if check is None else list(check)
        self.first_block = np.concatenate([[0], np.cumsum([len(bl) for bl in blocks])]).astype(np.int64)
        self.oracle = {i: oracle.phase_blocks(pileups[i], [s for s, _ in blocks[i]], [e for _, e in blocks[i]], oracle.make_params(eps, P, B), threads=4) for i in self.check}

    def check_oracle(self, r, what):
        ro_all = r.read_off.astype(np.int64)
        for i, o in self.oracle.items():
            b0, b1 = int(self.first_block[i]), int(self.first_block[i + 1])
            assert np.array_equal(o.best_ploidy, r.best_ploidy[b0:b1]), (what, i, o.best_ploidy, r.best_ploidy[b0:b1])
            assert np.array_equal(o.ploidies_tried, r.ploidies_tried[b0:b1]), (what, i)
            assert np.array_equal(o.mec.view(np.uint64), r.mec[b0:b1].view(np.uint64)), (what, i, o.mec, r.mec[b0:b1])
            lo, hi = int(ro_all[b0]), int(ro_all[b1])
            assert np.array_equal(np.diff(o.read_off.astype(np.int64)), np.diff(ro_all[b0:b1 + 1])), (what, i)
            assert np.array_equal(o.read_id, r.read_id[lo:hi]) and np.array_equal(o.part, r.part[lo:hi]), (what, i)
        if len(self.oracle) == len(self.pileups):
            assert min(o.min_prune_margin for o in self.oracle.values()) == r.min_prune_margin, what


def same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"
    assert a.mec.shape == b.mec.shape and np.array_equal(a.mec.view(np.uint64), b.mec.view(np.uint64)), f"{what}: mec"
    assert a.min_prune_margin == b.min_prune_margin, f"{what}: min_prune_margin"


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


def both_ways(ctx, lib, case, knobs, what, packed=True, contigs=None, **more):
    """the case with and without the option: equal to each other, equal to the oracle, and the packed stream taken exactly where `packed` says"""
    own = contigs is None
    res = ctx.upload_batch(case.pileups) if own else contigs
    out = []
    try:
        knobs(speculate=0, opt_threads=512, **more)
        for pk in COMBOS:
            knobs(opt_packed=pk)
            r = ctx.phase_blocks_batch(res, case.bc, case.bs, case.be, lib.make_params(case.eps, case.P, case.B))
            t = ctx.timing()
            assert t["optimize_launches"] > 0, what
            want = t["optimize_launches"] if (pk and packed) else 0
            assert t["optimize_packed_launches"] == want, (what, pk, t["optimize_packed_launches"], t["optimize_launches"])
            out.append(r)
    finally:
        if own:
            for x in res:
                x.free()
    same_bits(out[0], out[1], f"{what}: opt_packed=0 against the default")
    for pk, r in zip(COMBOS, out):
        case.check_oracle(r, f"{what}: opt_packed={pk}")
    return out[0]


def planted_reads(rng, n_snps, strains, lengths, lo=0, alleles=2, err=0.04, quals=None, max_start=None):
    """one read of exactly L consecutive cells per entry of `lengths`, of a random strain, anywhere it fits (first SNP <= max_start)"""
    hap = rng.integers(0, alleles, size=(strains, n_snps))
    reads = []
    for L in lengths:
        hi = n_snps - L + 1 if max_start is None else min(n_snps - L + 1, max_start)
        s = int(rng.integers(1, hi + 1))
        snps = np.arange(s, s + L)
        al = hap[int(rng.integers(0, strains)), snps - 1].copy()
        flip = rng.random(L) < err
        al[flip] = rng.integers(0, alleles, size=int(flip.sum()))
        q = rng.integers(8, 41, size=L) if quals is None else rng.choice(quals, size=L)
        reads.append((snps + lo, al, q))
    return reads


LENGTHS = [1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257]


@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_read_lengths_and_first_cell_offsets(gpu_ctx, hip_lib, oracle_mod, knobs, a):
    # every length three times and 24 reads of 20-40 cells, all starting at SNP <= 280 of 300; then one filler read that brings the cell count to a (mod 4) and the
    # contig's LAST read (the only one that starts past SNP 280: Frag order puts it last), five cells from offset a (mod 4) to the very end of the array.  One
    # contig per batch: its arrays start the arena's 256-byte aligned regions, so a cell's index mod 4 is its address mod 16 bytes over four.
    rng = np.random.default_rng(7700 + a)
    reads = planted_reads(rng, 300, 3, LENGTHS * 3 + list(rng.integers(20, 41, size=24)), max_start=280)
    cells = sum(len(s) for s, _, _ in reads)
    reads += planted_reads(rng, 300, 3, [4 + (a - cells) % 4], max_start=280)
    hap_last = rng.integers(0, 2, size=5)
    reads.append((np.arange(296, 301), hap_last, np.full(5, 30)))
    p = Pileup.from_reads(reads)
    assert int(p.first[-1]) == 296 and int(p.read_off[-2]) % 4 == a and int(p.read_off[-1]) == p.n_cells and p.n_cells % 4 == (a + 5) % 4
    assert set(int(x) % 4 for x in p.read_off[:-1]) == {0, 1, 2, 3}
    lens = np.diff(p.read_off.astype(np.int64))
    assert set(LENGTHS) <= set(int(x) for x in lens)
    c = Case(oracle_mod, [p], [[(1, 300)]])
    assert int(np.diff(c.oracle[0].read_off.astype(np.int64))[0]) == p.n_reads, "the block does not hold every read"
    both_ways(gpu_ctx, hip_lib, c, knobs, f"lengths, last read at offset {a} (mod 4)")


def test_reads_per_block_around_the_lane_groups(gpu_ctx, hip_lib, oracle_mod, knobs):
    # one contig per read count, one block each; the contigs share an arena, so their arrays start at whatever offset the contigs before them leave
    rng = np.random.default_rng(7710)
    counts = [1, 15, 16, 17, 31, 32, 33]
    piles = [Pileup.from_reads(planted_reads(rng, 24, 2, list(rng.integers(3, 14, size=n)))) for n in counts]
    c = Case(oracle_mod, piles, [[(1, 24)]] * len(counts))
    assert [int(np.diff(c.oracle[i].read_off.astype(np.int64))[0]) for i in range(len(counts))] == counts
    both_ways(gpu_ctx, hip_lib, c, knobs, "blocks of 1 .. 33 reads")


def test_quality_bytes_at_the_ends_of_the_weight_table(gpu_ctx, hip_lib, oracle_mod, knobs):
    # q = 0 weighs nothing (the call's beam kernels are the q0 instances; the optimise kernel has no such split), q = 72 .. 76 are the last steps below 2^24, from
    # q = 76 on the weight is 2^24
    rng = np.random.default_rng(7720)
    quals = [0, 1, 72, 73, 75, 76, 93, 255]
    piles = [Pileup.from_reads(planted_reads(rng, 40, st, list(rng.integers(2, 15, size=60)), quals=quals)) for st in (1, 2, 3)]
    assert set(quals) <= set(int(q) for p in piles for q in p.qual)
    c = Case(oracle_mod, piles, [[(1, 14), (11, 24), (21, 40)]] * 3)
    both_ways(gpu_ctx, hip_lib, c, knobs, "quality bytes 0, 1, 72, 73, 75, 76, 93, 255")


def test_four_alleles_stay_on_the_wide_cells(gpu_ctx, hip_lib, oracle_mod, knobs):
    rng = np.random.default_rng(7730)
    piles = [Pileup.from_reads(planted_reads(rng, 40, st, list(rng.integers(2, 15, size=60)), alleles=4)) for st in (2, 3)]
    assert set(int(x) for p in piles for x in p.allele) == {0, 1, 2, 3}
    c = Case(oracle_mod, piles, [[(1, 14), (11, 24), (21, 40)]] * 2)
    both_ways(gpu_ctx, hip_lib, c, knobs, "alleles 0-3", packed=False)          # (the four-allele instances read the 8-byte cells)


def test_snp_indices_past_65536(gpu_ctx, hip_lib, oracle_mod, knobs):
    # small deltas on large absolute indices: the packed cell holds the distance to the read's first SNP, the block's base comes from the read's metadata
    rng = np.random.default_rng(7740)
    lo = 70000
    piles = [Pileup.from_reads(planted_reads(rng, 60, st, list(rng.integers(2, 30, size=70)), lo=lo)) for st in (2, 3)]
    assert min(int(p.snp.min()) for p in piles) > 65536
    c = Case(oracle_mod, piles, [[(lo + 1, lo + 25), (lo + 20, lo + 45), (lo + 40, lo + 60)]] * 2)
    both_ways(gpu_ctx, hip_lib, c, knobs, "SNP indices past 65 536")


@pytest.fixture(scope="module")
def strains(oracle_mod):
    # contigs of 1 / 2 / 3 / 4 strains (the first with an error rate far below epsilon), four blocks each: blocks that stop at ploidy 1 and blocks that reach ploidy >= 3
    rng = np.random.default_rng(7750)
    piles = [random_pileup(rng, 60, 40, st, max_len=14, err=er, drop=0.05) for st, er in zip((1, 2, 3, 4), (0.002, 0.02, 0.02, 0.02))]
    blocks = [[(s, min(40, s + 13)) for s in range(1, 41, 10)]] * 4
    return piles, blocks


@pytest.mark.parametrize("fuse_p1", [0, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_every_ploidy_with_and_without_the_fused_ploidy_1(gpu_ctx, hip_lib, oracle_mod, knobs, strains, P, fuse_p1):
    piles, blocks = strains
    c = Case(oracle_mod, piles, blocks, P=P)
    tried = np.concatenate([c.oracle[i].ploidies_tried for i in range(4)])
    assert (tried == 1).any() and (tried == min(P, 3)).any(), tried
    both_ways(gpu_ctx, hip_lib, c, knobs, f"max_ploidy {P}, fuse_p1 {fuse_p1}", fuse_p1=fuse_p1)


def _last_round_was_rejected(pile, oracle, start, end, ploidy):
    """Does the optimisation of this (block, ploidy) job end with a round whose moves are undone?  The oracle's partition after optimisation is the last accepted one; if
    opt_iterate (the Python restatement's) still moves reads from it and fewer than 20 rounds ran, the last round made those moves and was rejected."""
    from oracle import py_restatement as pr
    rid, _, po, _, _, iters = oracle.one_ploidy(pile, start, end, ploidy, EPS)
    if iters >= 20:
        return False, iters
    frags = pr.frags_from_pileup(pile)
    part = [set(frags[int(r)] for r, k in zip(rid, po) if k == q) for q in range(ploidy)]
    moved = pr.opt_iterate(part, pr.hap_block_from_partition(part, True), EPS)
    return any(a != b for a, b in zip(moved, part)), iters


def test_several_rounds_and_a_rejected_round(gpu_ctx, hip_lib, oracle_mod, knobs):
    # seeded search (on the CPU) for a block whose optimisation at some ploidy accepts at least two rounds and one whose last round is rejected (the undo path)
    found_rounds = found_rejected = None
    for seed in range(7760, 7800):
        rng = np.random.default_rng(seed)
        pile = random_pileup(rng, 70, 30, 3, max_len=16, err=0.12, drop=0.1)
        for ploidy in (2, 3):
            rejected, iters = _last_round_was_rejected(pile, oracle_mod, 1, 30, ploidy)
            if found_rounds is None and iters >= 3:
                found_rounds = pile
            if found_rejected is None and rejected:
                found_rejected = pile
        if found_rounds is not None and found_rejected is not None:
            break
    assert found_rounds is not None, "no seed gives a block with three optimise rounds"
    assert found_rejected is not None, "no seed gives a block whose last optimise round is rejected"
    c = Case(oracle_mod, [found_rounds, found_rejected], [[(1, 30)]] * 2)
    both_ways(gpu_ctx, hip_lib, c, knobs, "several rounds / a rejected round")


def test_a_device_assembled_contig_in_the_call_takes_the_wide_cells(gpu_ctx, hip_lib, oracle_mod, knobs):
    # contig 1 is made on the device by floria_hip_drop_monomorphic, whose output carries no packed cells: the call over {uploaded contig, device-made contig} reads the
    # 8-byte cells for both and still agrees with the oracle (which phases the numpy model's filtered pileup); the same two pileups uploaded take the packed stream
    from tests import mono_model as mm
    rng = np.random.default_rng(7770)
    piles = [random_pileup(rng, 60, 40, 2, max_len=14, err=0.02, drop=0.05) for _ in range(2)]
    filtered = mm.drop_monomorphic(piles[1], 40, 0.001)[0]
    assert filtered.n_reads >= 30
    blocks = [[(s, min(40, s + 13)) for s in range(1, 41, 10)]] * 2
    c = Case(oracle_mod, [piles[0], filtered], blocks)
    up = gpu_ctx.upload_batch(piles)
    try:
        batch, res = gpu_ctx.drop_monomorphic([up[1]], [40], 0.001)
        try:
            assert int(res["read_off"][-1]) == filtered.n_reads
            made = hip_lib.ResidentContig(gpu_ctx, handle=hip_lib.C.c_void_p(batch._arr[0]), n_reads=filtered.n_reads)
            try:
                both_ways(gpu_ctx, hip_lib, c, knobs, "uploaded + device-made contig", packed=False, contigs=[up[0], made])
            finally:
                made._h = None          # owned by `batch`
        finally:
            batch.free()
    finally:
        for x in up:
            x.free()
    both_ways(gpu_ctx, hip_lib, c, knobs, "both contigs uploaded", packed=True)


def test_seeded_sweep_of_medium_pileups(gpu_ctx, hip_lib, oracle_mod, knobs):
    # 200 random pileups (120-200 reads over 60-90 SNPs, reads up to 48 cells, 1-4 strains, error 1-10 %) in one batch, three overlapping blocks each; with and
    # without the option on all of them, the oracle on every eighth contig
    rng = np.random.default_rng(7780)
    piles, blocks = [], []
    for _ in range(200):
        n_snps = int(rng.integers(60, 91))
        piles.append(random_pileup(rng, int(rng.integers(120, 201)), n_snps, int(rng.integers(1, 5)), max_len=48, err=float(rng.uniform(0.01, 0.1)), drop=0.1))
        blocks.append([(1, n_snps // 2), (n_snps // 3, 2 * n_snps // 3 + 5), (n_snps // 2, n_snps)])
    c = Case(oracle_mod, piles, blocks, check=range(0, 200, 8))
    r = both_ways(gpu_ctx, hip_lib, c, knobs, "sweep")
    assert len(set(int(x) for x in r.best_ploidy)) >= 3, "the sweep's blocks all end at the same ploidy"
