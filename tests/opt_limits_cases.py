"""The inputs of tests/test_gpu_opt_limits.py — blocks at the size limits of the optimise kernel's packed and delta instances — built in one place, so that
tests/test_opt_limits_cpu.py can assert on the CPU, with tests/opt_plan_model.py, the oracle and tests/opt_delta_model.py, that every case is what its name says
before the GPU file runs the very same arrays.

Every contig carries ONE block over all of its reads, (1, last SNP).  A block's span is last position - first position + 1 over its reads (blocks_kernel.h); where a
case needs an exact span, one read is pinned to SNP 1 and one to the last SNP."""
import numpy as np

from floria_amd.pileup import Pileup
from tests import opt_delta_model as model
from tests import opt_plan_model as plan
from tests.test_gpu_opt_packed import planted_reads

EPS = 0.03125
NARROW = 60          # SNPs of the narrow blocks of (a), (d), (f)


class Spec:
    """a call: contigs (one block each), max_ploidy, alleles"""

    def __init__(self, name, pileups, P=5, alleles=2):
        self.name, self.pileups, self.P, self.alleles = name, list(pileups), P, alleles

    def blocks(self):
        return [[(1, int(p.snp.max()))] for p in self.pileups]

    def shapes(self):
        """(reads, span) of every block"""
        return [(p.n_reads, int(p.last.max()) - int(p.first.min()) + 1) for p in self.pileups]

    def plan(self, **kw):
        return plan.plan_for_blocks(self.shapes(), self.alleles, self.P, **kw)

    def sub(self, name, contigs):
        return Spec(name, [self.pileups[i] for i in contigs], self.P, self.alleles)


def pinned(rng, n_snps, L=20, alleles=2):
    """two reads of L cells: one from SNP 1, one up to SNP n_snps"""
    return [(np.arange(1, L + 1), rng.integers(0, alleles, size=L), rng.integers(8, 41, size=L)),
            (np.arange(n_snps - L + 1, n_snps + 1), rng.integers(0, alleles, size=L), rng.integers(8, 41, size=L))]


def narrow_block(seed, n_reads, alleles=2, strains=3, err=0.12):
    """n_reads reads of 3-12 cells over 60 SNPs, three planted strains"""
    rng = np.random.default_rng(seed)
    reads = planted_reads(rng, NARROW, strains, list(rng.integers(3, 13, size=n_reads - 2)), alleles=alleles, err=err) + pinned(rng, NARROW, 8, alleles)
    return Pileup.from_reads(reads)


def wide_block(seed, n_reads, span, strains, err=0.04):
    """n_reads reads of 20-60 cells over exactly `span` SNPs"""
    rng = np.random.default_rng(seed)
    return Pileup.from_reads(planted_reads(rng, span, strains, list(rng.integers(20, 61, size=n_reads - 2)), err=err) + pinned(rng, span))


# ---- (a) reads per block around 512 and 1024 ----------------------------------------------------------------------------------------------------------
A_COUNTS = [511, 512, 513, 1023, 1025]
# The seeds of the blocks of more than 512 reads were searched (once, on the CPU: seeds 20000-22999 for 513 reads — 20075, 21499 and 22298 are the hits: a single late
# read seldom decides anything —, 9400-9439 for 1 023 and 1 025) for blocks on which a delta pass that stops at read 512 changes a PARTITION, not just a distance:
# `broken_delta_leaves_oracle` below, which tests/test_opt_limits_cpu.py asserts.  A flip inside the span of a late read is not enough for a test to notice — the
# stale distance must also decide a move.
A_SEEDS = {511: 9911, 512: 9912, 513: 20075, 1023: 9409, 1025: 9402}


def case_a(counts=A_COUNTS):
    return Spec("a: " + " / ".join(str(n) for n in counts) + " reads", [narrow_block(A_SEEDS[n], n) for n in counts])


# ---- (b) candidate lists on both sides of OPT_SORT_LDS --------------------------------------------------------------------------------------------------
# A round has M candidate moves when M (read, other partition) pairs have a positive gain.  The beam search hands the optimiser a partition that is close to a local
# optimum, so on planted random data M stays far below 512: seeded searches over blocks of 360-380 reads (40-170 SNPs, 3-8 strains, error 0.1-0.6, reads of 1-40
# cells, a beam of 1 or 10: 148 blocks) found no round above M = 108, and 104 blocks of 2 000 / 4 000 reads none above M = 297.  The blocks here are CONSTRUCTED instead,
# around the one thing the beam cannot see: it scores a read against the reads before it (Frag order: first position ascending), the optimiser against all of them.
#   SNP 1 a dummy, SNP 2 "x", SNPs 3-6 the payload, SNPs 7-18 twelve anchors (four code words, pairwise distance 6)
#   G1  four heavy reads (q 40) over {1, 3..18}: anchors c_k, payload P_k — they open the four partitions
#   G2  light reads (q 1; q 2 in group 0) over {2..6}: payload P_k, so they join partition k
#   G3  heavy reads over {3..18}: anchors c_k, payload ~P_k — four mismatches in partition k, six anywhere else: they join k and turn its payload consensus to ~P_k
# Afterwards every light read is at distance 4 w from its own partition and at (4 - |P_k - P_j|) w from partition j: three candidates each, M = 3 x (light reads).
# The heavier light reads of group 0 head the sorted list and are exactly the M / 10 + 2 moves of round 0; they all go to the partition with the complementary
# payload, which leaves SNP x of their old partition empty: ONE flipped code byte behind a pool-sorted round, so round 1 opens with a delta pass — and has
# 3 x (the other light reads) candidates: 510 in the first block, 513 in the second.
B_ANCHORS = ["000000000000", "111111000000", "000111111000", "111000111000"]
B_PAYLOADS = ["0000", "1111", "0011", "1100"]
B_LIGHT = [[75, 57, 57, 56], [75, 57, 57, 57]]          # light reads per group; 75 = (3 x 245) // 10 + 2 = (3 x 246) // 10 + 2
B_HEAVY = [34, 16, 16, 16]                                # G3 reads per group: they outweigh the group's light reads (75 x w(2) = 27.7, 57 x w(1) = 11.7)


def b_block(light):
    bits = lambda s: np.array([int(c) for c in s])
    apos, ppos = np.arange(7, 19), np.arange(3, 7)
    reads = []
    for k in range(4):
        reads.append((np.concatenate([[1], ppos, apos]), np.concatenate([[0], bits(B_PAYLOADS[k]), bits(B_ANCHORS[k])]), np.full(17, 40)))
    for k in range(4):
        reads += [(np.concatenate([[2], ppos]), np.concatenate([[0], bits(B_PAYLOADS[k])]), np.full(5, 2 if k == 0 else 1))] * light[k]
    for k in range(4):
        reads += [(np.concatenate([ppos, apos]), np.concatenate([1 - bits(B_PAYLOADS[k]), bits(B_ANCHORS[k])]), np.full(16, 40))] * B_HEAVY[k]
    return Pileup.from_reads(reads)


def case_b():
    return Spec("b: candidate lists around OPT_SORT_LDS", [b_block(light) for light in B_LIGHT])


# ---- (c) the HL edge at ploidy 3 ------------------------------------------------------------------------------------------------------------------------
C_READS, C_SEED, C_STRAINS = 100, 9600, 5


def case_c(extra):
    """extra = 0: the largest span that is HL at ploidy 3 with 100 reads (five planted strains, so that the reference goes on to ploidy 4); 1: one SNP more"""
    span = plan.largest_hl_span(C_READS, 3) + extra
    return Spec(f"c: span {span} (largest HL span at ploidy 3 + {extra})", [wide_block(C_SEED, C_READS, span, C_STRAINS, err=0.08)])


# ---- (d) n_max / span_max decide for the whole batch ------------------------------------------------------------------------------------------------------
D_READS, D_SEED = 100, 9700


def case_d(batch):
    """the narrow block alone, or in a batch with a contig whose block has the largest span that is HL at ploidy 2 (and no more reads)"""
    piles = [narrow_block(D_SEED, D_READS)]
    if batch:
        piles.append(wide_block(D_SEED + 1, D_READS, plan.largest_hl_span(D_READS, 2), 2))
    return Spec("d: narrow block " + ("beside a wide one" if batch else "alone"), piles)


# ---- (e) OPT_META_MAX -------------------------------------------------------------------------------------------------------------------------------------
E_SEED, E_SNPS = 9800, 300


def case_e(n_reads):
    rng = np.random.default_rng(E_SEED)
    reads = planted_reads(rng, E_SNPS, 3, list(rng.integers(3, 7, size=n_reads - 2)), err=0.08) + pinned(rng, E_SNPS, 6)
    return Spec(f"e: {n_reads} reads", [Pileup.from_reads(reads)])


# ---- (f) four alleles ---------------------------------------------------------------------------------------------------------------------------------------
def case_f():
    return Spec("f: four alleles, 513 reads", [narrow_block(9900, 513, alleles=4)], alleles=4)


# ---- the model's account of a case ----------------------------------------------------------------------------------------------------------------------------
def account(oracle, pile, tried, ploidies, w24=None):
    """the optimise rounds of the block's jobs at `ploidies` (those the reference runs: 2 .. tried), restated: -> {"passes", "fallbacks", "rounds": {p: [...]},
    "reads": [(first, last) relative to the block, in block order]}; the model is pinned to the oracle on the way"""
    w24 = oracle.weight_q24() if w24 is None else w24
    end = int(pile.snp.max())
    out = {"passes": 0, "fallbacks": 0, "rounds": {}}
    pos0 = int(pile.first.min())
    out["reads"] = [(int(f) - pos0, int(l) - pos0) for f, l in zip(pile.first, pile.last)]
    for p in ploidies:
        if p < 2 or p > tried:
            continue
        rid, pb, po, _, _, iters = oracle.one_ploidy(pile, 1, end, p, EPS)
        assert np.array_equal(rid, np.arange(pile.n_reads)), "the block does not hold every read in order"
        part, it, rounds = model.run(pile, rid, pb, p, EPS, w24)
        assert np.array_equal(part, po) and it == iters, ("the model left the oracle", p, it, iters)
        out["rounds"][p] = rounds
        out["passes"] += sum(r["pass"] == "delta" for r in rounds)
        out["fallbacks"] += sum(r["pass"] == "interval" for r in rounds)
    return out


def predict(oracle, spec, tried, pl):
    """delta passes / fallbacks of the call: every job at the ploidies whose plan keeps integer distances"""
    w24 = oracle.weight_q24()
    delta_p = [p for p in range(2, spec.P + 1) if pl[p]["delta"]]
    acc = [account(oracle, spec.pileups[i], int(tried[i]), delta_p, w24) for i in range(len(spec.pileups))]
    return sum(a["passes"] for a in acc), sum(a["fallbacks"] for a in acc), acc


def broken_delta_leaves_oracle(oracle, pile, tried, limit):
    """would a kernel whose delta pass visits only the first `limit` reads of this block end with another partition at some ploidy the call runs?"""
    w24, end = oracle.weight_q24(), int(pile.snp.max())
    for p in range(2, tried + 1):
        rid, pb, po, _, _, _ = oracle.one_ploidy(pile, 1, end, p, EPS)
        if not np.array_equal(model.run(pile, rid, pb, p, EPS, w24, delta_reads=limit)[0], po):
            return True
    return False


def flip_reaches_read_from(acc, first_index):
    """does some delta pass of this account exchange a term in the span of a read whose index in the block is >= first_index?"""
    late = acc["reads"][first_index:]
    for rounds in acc["rounds"].values():
        for r in rounds:
            if r["pass"] == "delta" and any(f0 <= fl[0] <= l0 for fl in r["flips"] for f0, l0 in late):
                return True
    return False
