"""Seeded worlds at large SNP indices and wide blocks, shared by tests/test_wide_cases_cpu.py and tests/test_gpu_wide.py (nothing on disk).

A world is a pileup, its block ranges and the -p / -n it is run with.  `shifted(world, k)` is the same world k SNPs further along its contig: the
state hash wraps the absolute SNP index at 65 536 (csrc/common.h: hash_idx), and the reference arithmetic emulates hash containers keyed by it, so a
moved world is the same input for the canonical arithmetic and a new one for the reference arithmetic.
"""
from dataclasses import dataclass, replace

import numpy as np

from floria_amd.pileup import Pileup, reads_in_interval
from tests.helpers import random_pileup

HASH_M = 65536                 # csrc/common.h
K_FAR = 3 * HASH_M + 1
K_CHROM = 5_000_000
READ_SPAN_MAX = 10000          # blocks_kernel.h: `last - first <= 10000`


@dataclass
class World:
    pile: Pileup
    s: np.ndarray              # block ranges, 1-based inclusive
    e: np.ndarray
    P: int
    B: int

    @property
    def S(self):
        return int(self.pile.last.max())


def k_wrap(world):
    """K_WRAP of a world: moved by it, a block that covers the middle of the world straddles SNP index 65 536."""
    return HASH_M - world.S // 2


def offsets(world):
    return {"wrap": k_wrap(world), "far": K_FAR, "chrom": K_CHROM}


def shifted(x, k):
    """The pileup (or the world: pileup and block ranges) with every SNP index moved by k."""
    if isinstance(x, World):
        return replace(x, pile=shifted(x.pile, k), s=(x.s.astype(np.int64) + k).astype(np.uint32), e=(x.e.astype(np.int64) + k).astype(np.uint32))
    mv = lambda a: (np.asarray(a, np.int64) + int(k)).astype(np.uint32)
    return Pileup(x.read_off.copy(), mv(x.snp), x.allele.copy(), x.qual.copy(), mv(x.first), mv(x.last), None if x.set_order is None else x.set_order.copy())


def block_extent(pile, start, end):
    """(pos0, span, read ids) of a block as csrc/blocks_kernel.h computes them: min first and max last over the reads that pass."""
    ids = reads_in_interval(pile, start, end)
    if len(ids) == 0:
        return 0, 0, ids
    lo, hi = int(pile.first[ids].min()), int(pile.last[ids].max())
    return lo, hi - lo + 1, ids


def dup_world(seed):
    """The cloned-read pileups of tests/test_gpu_parity.py (test_general_insert_path_duplicates_and_ties): duplicates with equal scores in almost every
    step, so the state hash decides the result.  Two overlapping blocks, -p 5, -n 10 / 4 / 7."""
    from tests.test_gpu_parity import _cloned_reads_pileup
    rng = np.random.default_rng(8800 + seed)
    pile = _cloned_reads_pileup(rng, 40 + 10 * (seed % 4), 12, 60, 2 + seed % 3)
    S = int(pile.last.max())
    return World(pile, np.array([1, S // 2], np.uint32), np.array([S, S], np.uint32), 5, [10, 10, 4, 7][seed % 4])


def medium_world(seed, small=False):
    """Hundreds of reads over 40 .. 300 SNPs; one seed in three has four alleles, one in four q = 0 cells.  Two overlapping blocks, -p 5 -n 10.
    small: 80 reads of at most 14 cells over 40 SNPs (a size the Python restatement runs in a second or two)."""
    rng = np.random.default_rng(31000 + seed)
    n_reads, n_snps, ploidy, max_len = int(rng.integers(150, 501)), int(rng.integers(40, 301)), int(rng.integers(2, 5)), int(rng.integers(5, 81))
    if small:
        n_reads, n_snps, max_len = 80, 40, 14
    pile = random_pileup(rng, n_reads, n_snps, ploidy, max_len=max_len,
                         alleles=4 if seed % 3 == 2 else 2, q0_frac=0.08 if seed % 4 == 1 else 0.0, err=float(rng.choice([0.03, 0.08])))
    S = int(pile.last.max())
    return World(pile, np.array([1, max(1, S // 3)], np.uint32), np.array([max(1, 2 * S // 3), S], np.uint32), 5, 10)


LONG_SPANS = (10001, 10002, 4096, 4097, 4095)       # SNPs from first to last of the dense reads, in turn


def long_world():
    """36 reads of two strains over 12 000 SNPs.  Five in six are dense (a cell at every SNP of their span), spans LONG_SPANS in turn: 10 001 is the longest
    read a block takes, 10 002 is left out, and 4 096 cells is where the 32-bit first-insertion keys of the reference arithmetic end.  Every sixth read has
    300 cells scattered over 6 000 SNPs.  3 % errors, q in 10 .. 40; blocks [1, 12000] and [3000, 9000], -p 3 -n 5."""
    rng = np.random.default_rng(12000)
    n_snps = 12000
    hap = rng.integers(0, 2, size=(2, n_snps))
    reads, dense = [], 0
    for i in range(36):
        if i % 6 == 5:
            first = int(rng.integers(1, n_snps - 6000 + 2))
            snps = np.sort(np.concatenate([[first, first + 5999], rng.choice(np.arange(first + 1, first + 5999), size=298, replace=False)]))
        else:
            span = LONG_SPANS[dense % 5]; dense += 1
            first = int(rng.integers(1, n_snps - span + 2)) if span > 10000 else int(rng.integers(1000, 7001))
            snps = np.arange(first, first + span)
        al = hap[i % 2, snps - 1].copy()
        flip = rng.random(len(snps)) < 0.03
        al[flip] ^= 1
        reads.append((snps, al, rng.integers(10, 41, size=len(snps))))
    pile = Pileup.from_reads(reads)
    return World(pile, np.array([1, 3000], np.uint32), np.array([n_snps, 9000], np.uint32), 3, 5)


def span_limit_world(extra=0, alleles=2, n_reads=900):
    """About 900 sparse reads (2 .. 40 cells, at most 10 001 SNPs from first to last) of two strains and ONE block whose reads start at `pos0` and end at
    pos0 + 65535 + extra: extra = 0 is the widest block the library takes (span 65 536 = the period of the state hash), extra = 1 the first it refuses.
    Three cells in four sit on a lattice of every 61st SNP, so that positions are shared by many reads.  -p 2 -n 3."""
    rng = np.random.default_rng(65536 + alleles)
    pos0 = 1000
    end = pos0 + HASH_M - 1 + extra
    hap = rng.integers(0, alleles, size=(2, HASH_M + 2))

    def read(first, last, k, strain):
        inner = np.arange(first + 1, last)
        lattice = inner[(inner - pos0) % 61 == 0]
        n_in = max(0, min(k - 2, len(inner)))
        n_lat = min(len(lattice), (3 * n_in) // 4)
        pick = np.concatenate([rng.choice(lattice, size=n_lat, replace=False), rng.choice(inner, size=n_in - n_lat, replace=False)]) if n_in else np.zeros(0, np.int64)
        snps = np.unique(np.concatenate([[first, last], pick])).astype(np.int64)
        al = hap[strain, snps - pos0].copy()
        flip = rng.random(len(snps)) < 0.04
        al[flip] = rng.integers(0, alleles, size=int(flip.sum()))
        return snps, al, rng.integers(10, 41, size=len(snps))

    reads = [read(pos0, pos0 + 9000, 30, 0), read(end - READ_SPAN_MAX, end, 30, 1)]          # the two anchors: the block's first and last SNP
    for i in range(n_reads - 2):
        span = int(rng.integers(500, READ_SPAN_MAX + 2))                                       # SNPs from first to last, <= 10 001
        first = int(rng.integers(pos0, pos0 + HASH_M - span + 1))                             # last <= pos0 + 65535
        reads.append(read(first, first + span - 1, int(rng.integers(2, 41)), i % 2))
    pile = Pileup.from_reads(reads)
    return World(pile, np.array([pos0], np.uint32), np.array([end], np.uint32), 2, 3)
