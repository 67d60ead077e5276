"""Inputs shared by tests/test_gpu_join_paths.py and tests/test_gpu_reassign_from_handle.py: small S1 batches and path lists built FROM their results, so that no case
can go vacuous (every builder asserts the phenomenon it is there for).

sized_world()   five contigs in one S1 call:
                  0  long reads (floria_amd/synth.py), 400 reads, 600 SNPs: four overlapping blocks, and three whose lists have exactly 64, 65 and 129 reads;
                  1  two runs of reads with a gap between them: a block in the gap is empty;
                  2  5 000 long reads over 300 SNPs: a block at either end, a path over both has a window of more than 64 x 64 ids;
                  3  a small contig that gets no path;
                  4  a small contig.
random_world()  the 300 sparse contigs of tests/haploset_model.py (random_contig(seed)), two or three overlapping blocks each.
"""
import numpy as np

from floria_amd import synth
from tests import haploset_model as hm
from tests import join_model as jm

N_RANDOM = 300


def block_counts(p, s, e):
    return int(((p.first.astype(np.int64) <= e) & (p.last.astype(np.int64) >= s)).sum())


def find_block(p, n):
    """An SNP range whose block list (find_reads_in_interval) has exactly n reads."""
    S = int(p.last.max())
    for s in range(1, S + 1, 3):
        for e in range(s, S + 1):
            c = block_counts(p, s, e)
            if c == n:
                return s, e
            if c > n:
                break
    raise AssertionError(f"no block with {n} reads")


def sized_world():
    main = synth.make_contig(np.random.SeedSequence([20261020, 1]), 600, 400, 2, "long").pileup
    gap = hm.reads_pileup(hm.run_of(1, 30, 3) + hm.run_of(60, 30, 3))
    big = synth.make_contig(np.random.SeedSequence([20261020, 2]), 300, 5000, 2, "long").pileup
    none = synth.make_contig(np.random.SeedSequence([20261020, 3]), 200, 120, 2, "long").pileup
    small = synth.make_contig(np.random.SeedSequence([20261020, 4]), 200, 150, 3, "long").pileup
    assert big.n_reads > 4500
    blocks = []                                            # (contig, start, end)
    S = int(main.last.max())
    for s in range(1, S, 120):                             # overlapping by 60 SNPs
        blocks.append((0, s, min(S, s + 179)))
    sized = {}
    for n in (64, 65, 129):
        sized[n] = len(blocks)
        blocks.append((0,) + find_block(main, n))
    gap_blocks = len(blocks)
    blocks += [(1, 1, 20), (1, 40, 50), (1, 55, 80)]       # the middle one lies in the gap
    assert block_counts(gap, 40, 50) == 0 and block_counts(gap, 1, 20) > 0 and block_counts(gap, 55, 80) > 0
    big_blocks = len(blocks)
    Sb = int(big.last.max())
    blocks += [(2, 1, 12), (2, Sb - 11, Sb)]
    blocks += [(3, 1, 100), (3, 70, int(none.last.max()))]
    small_blocks = len(blocks)
    blocks += [(4, 1, 90), (4, 60, 150), (4, 120, int(small.last.max()))]
    b = np.asarray(blocks, np.uint32)
    return dict(pileups=[main, gap, big, none, small], bc=b[:, 0].copy(), bs=b[:, 1].copy(), be=b[:, 2].copy(), sized=sized, gap_blocks=gap_blocks,
                big_blocks=big_blocks, small_blocks=small_blocks, n_main_regular=sized[64])


def random_world():
    worlds = [hm.random_contig(seed) for seed in range(N_RANDOM)]
    pileups = [hm.reads_pileup(w[0]) for w in worlds]
    rng = np.random.default_rng(20261020)
    blocks = []
    for c, p in enumerate(pileups):
        S = int(p.last.max())
        nb = int(rng.integers(2, 4))
        step = max(1, S // nb)
        for i in range(nb):
            s = 1 + i * step
            blocks.append((c, s, S if i == nb - 1 else min(S, s + step + step // 3)))
    b = np.asarray(blocks, np.uint32)
    return dict(worlds=worlds, pileups=pileups, bc=b[:, 0].copy(), bs=b[:, 1].copy(), be=b[:, 2].copy())


def all_nodes(res):
    return [(b, k) for b in range(res.n_blocks) for k in range(int(res.best_ploidy[b]))]


def random_paths(res, bc, n_contigs, seed, max_paths=4):
    """Random node lists per contig (they need not be LP paths): up to max_paths paths a contig, each a random draw — with repeats across paths — of the contig's
    nodes; now and then an empty path.  -> path_contig, nodes, ranges"""
    rng = np.random.default_rng([20261020, seed])
    by_contig = [[] for _ in range(n_contigs)]
    for b, k in all_nodes(res):
        by_contig[int(bc[b])].append((b, k))
    path_contig, nodes, ranges = [], [], []
    for c in range(n_contigs):
        for _ in range(int(rng.integers(0, max_paths + 1))):
            pool = by_contig[c]
            n = int(rng.integers(0, min(len(pool), 5) + 1)) if pool else 0
            pick = [pool[i] for i in sorted(rng.choice(len(pool), n, replace=False))] if n else []
            lo = int(rng.integers(1, 50))
            path_contig.append(c); nodes.append(pick); ranges.append((lo, lo + int(rng.integers(0, 200))))
    return path_contig, nodes, ranges


def model_groups(res, nodes):
    return jm.join(res.read_off, res.read_id, res.part, nodes)


def per_contig(path_contig, groups, ranges, n_contigs):
    """-> per contig (groups, ranges), in path order"""
    out = [([], []) for _ in range(n_contigs)]
    for c, g, r in zip(path_contig, groups, ranges):
        out[c][0].append(g); out[c][1].append(tuple(int(x) for x in r))
    return out


def same_as_model(got, path_contig, groups, ranges, n_contigs, what=""):
    """got: Haplosets.download() -> assert it equals the model's groups, list for list"""
    want = per_contig(path_contig, groups, ranges, n_contigs)
    assert len(got) == n_contigs, what
    for c in range(n_contigs):
        g = got[c]
        assert g.n_groups == len(want[c][0]), f"{what} contig {c}: {g.n_groups} groups instead of {len(want[c][0])}"
        for i, w in enumerate(want[c][0]):
            assert np.array_equal(g.group(i), w), f"{what} contig {c} group {i}: {g.group(i)[:8]}.. instead of {w[:8]}.."
        assert [tuple(map(int, r)) for r in g.range] == want[c][1], f"{what} contig {c}: ranges"


def listed(groups_per_contig):
    """list of _capi.Groups in contig order -> grp_contig, groups, ranges of one call by arrays"""
    gc, groups, ranges = [], [], []
    for c, w in enumerate(groups_per_contig):
        for g in range(w.n_groups):
            gc.append(c); groups.append(w.group(g)); ranges.append(tuple(map(int, w.range[g])))
    return gc, groups, ranges
