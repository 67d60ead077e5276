"""Plain Python model of what follows S2's greedy re-insertion: the groups from the per-read assignment, separate_broken_haplogroups
(part_block_manip.rs:27-98) and sort_parts (:276-288), as floria_hip_reassign_batch computes them on the host and floria_hip_reassign_batch_resident on the device.

Two forms of the splits:
  epilogue()       the two walks, restated literally from the library's host code (the definition);
  epilogue_scan()  what csrc/haploset_kernel.h computes: an exclusive prefix maximum of `last`, a break flag per read, the part number as the count of breaks at or
                   before a read; a read with a break is dropped.
tests/test_haploset_cpu.py proves the two equal on random inputs and pins the first to the oracle.
"""
import numpy as np

U32_MAX = 0xFFFFFFFF


def groups_from_assign(assign, n_groups):
    """Group lg holds the reads with assign == lg, ascending by id."""
    parts = [[] for _ in range(n_groups)]
    for r, a in enumerate(assign):
        if a >= 0:
            parts[int(a)].append(r)
    return parts


def _sorted(parts, ranges, assign_only):
    idx = list(range(len(parts)))
    if not assign_only:
        idx.sort(key=lambda i: (ranges[i][0], ranges[i][1]))      # list.sort is stable, as std::stable_sort
    return [list(parts[i]) for i in idx], [tuple(ranges[i]) for i in idx]


def epilogue(first, last, parts, ranges, assign_only=False):
    """parts: read-id lists (ascending), ranges: (lo, hi) per part -> (parts, ranges) as the S2 call returns them."""
    parts = [list(p) for p in parts]
    ranges = [(int(a), int(b)) for a, b in ranges]
    if not assign_only:
        all_breaks = []
        for i, p in enumerate(parts):
            latest, breaks = 0, []
            for r in p:
                if latest != 0 and first[r] > latest and ranges[i][0] <= latest < ranges[i][1]:
                    breaks.append(latest)
                if last[r] > latest:
                    latest = int(last[r])
            if breaks:
                all_breaks.append((i, breaks))
        new_parts, new_ranges = [], []
        for i, breaks in all_breaks:
            spot, break_start, end_spot, cur = 0, ranges[i][0], breaks[0], []
            for r in parts[i]:
                if last[r] <= end_spot:
                    cur.append(r)
                else:                                              # this read is not re-inserted
                    new_parts.append(cur); cur = []
                    new_ranges.append((break_start, end_spot))
                    break_start = end_spot + 1
                    spot += 1
                    end_spot = breaks[spot] if spot != len(breaks) else U32_MAX
            new_parts.append(cur)
            new_ranges.append((break_start, ranges[i][1]))
        for i, _ in all_breaks:
            parts[i] = []
        parts += new_parts
        ranges += new_ranges
    return _sorted(parts, ranges, assign_only)


def epilogue_scan(first, last, parts, ranges, assign_only=False):
    """The same function in the form the kernels use."""
    ranges = [(int(a), int(b)) for a, b in ranges]
    out_parts = [list(p) for p in parts]
    out_ranges = list(ranges)
    if not assign_only:
        tail_parts, tail_ranges = [], []
        for i, p in enumerate(parts):
            lo, hi = ranges[i]
            l = np.asarray([int(last[r]) for r in p], np.int64)
            ex = np.concatenate([[0], np.maximum.accumulate(l)[:-1]]) if len(p) else np.zeros(0, np.int64)      # exclusive prefix maximum
            brk = np.asarray([ex[j] != 0 and int(first[r]) > ex[j] and lo <= ex[j] < hi for j, r in enumerate(p)], bool)
            nb = int(brk.sum())
            if nb == 0:
                continue
            part_no = np.cumsum(brk)                                # breaks at or before the read
            vals = [int(v) for v in ex[brk]]
            out_parts[i] = []
            for j in range(nb + 1):
                tail_parts.append([r for k, r in enumerate(p) if not brk[k] and part_no[k] == j])
                tail_ranges.append((lo if j == 0 else vals[j - 1] + 1, hi if j == nb else vals[j]))
        out_parts += tail_parts
        out_ranges += tail_ranges
    return _sorted(out_parts, out_ranges, assign_only)


def n_splits(first, last, parts, ranges):
    """Groups of `parts` that break."""
    n = 0
    for i, p in enumerate(parts):
        latest = 0
        for r in p:
            if latest != 0 and first[r] > latest and ranges[i][0] <= latest < ranges[i][1]:
                n += 1
                break
            latest = max(latest, int(last[r]))
    return n


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------------------------------------------
def reads_pileup(spans, rng=None):
    """A Pileup whose read r spans (first, last) = spans[r], cells at both ends (one cell where they coincide); spans must already be in Frag::cmp order."""
    from floria_amd.pileup import Pileup
    rng = rng or np.random.default_rng(1)
    reads = []
    for f, l in spans:
        snps = [f] if f == l else [f, l]
        reads.append((snps, rng.integers(0, 2, len(snps)), rng.integers(10, 40, len(snps))))
    p = Pileup.from_reads(reads)
    assert [(int(a), int(b)) for a, b in zip(p.first, p.last)] == [tuple(s) for s in spans], "spans are not in Frag::cmp order"
    return p


def run_of(first_at, n, width=0):
    """n reads (f, f + width) with f = first_at, first_at + 1, ...: every read overlaps or touches the next (no gap when width >= 1)."""
    return [(first_at + i, first_at + i + width) for i in range(n)]


def hand_cases():
    """name -> (spans, groups, ranges): DISJOINT groups, so every read has one candidate and the re-insertion assigns it there: the epilogue's input is exact."""
    C = {}
    # reads 0,1 cover 1..4; read 2 starts behind a gap at 7
    C["one_gap"] = ([(1, 3), (2, 4), (7, 9), (8, 10)], [[0, 1, 2, 3]], [(1, 10)])
    C["two_gaps"] = ([(1, 3), (2, 4), (7, 9), (8, 10), (13, 15), (14, 16)], [[0, 1, 2, 3, 4, 5]], [(1, 20)])
    C["latest_eq_hi"] = ([(1, 4), (7, 9)], [[0, 1]], [(1, 4)])                    # latest == hi: no break
    C["latest_eq_lo"] = ([(1, 4), (7, 9)], [[0, 1]], [(4, 12)])                   # latest == lo: break
    C["latest_lt_lo"] = ([(1, 4), (7, 9)], [[0, 1]], [(5, 12)])                   # latest < lo: no break
    C["bridge"] = ([(1, 40), (2, 4), (7, 9), (13, 15)], [[0, 1, 2, 3]], [(1, 40)])      # the first read bridges every later gap
    C["empty_group"] = ([(1, 3), (2, 4)], [[0, 1], []], [(1, 4), (2, 9)])
    # equal ranges keep their order; the new parts (1..4) and (5..10) of group 2 sort between / around the old groups
    C["stable"] = ([(1, 3), (1, 2), (2, 4), (7, 9)], [[0], [1], [2, 3]], [(1, 6), (1, 6), (1, 10)])
    C["part_between"] = ([(1, 4), (2, 3), (7, 9), (8, 8)], [[1], [0, 2], [3]], [(1, 3), (1, 10), (6, 9)])
    for n, at in ((64, 63), (65, 63), (65, 64), (129, 63), (129, 64), (129, 128)):      # the running maximum carried across a tile of 64 reads
        spans = run_of(1, at, 1) + run_of(at + 10, n - at, 1)
        C[f"tile_{n}_{at}"] = (spans, [list(range(n))], [(1, n + 20)])
    for ng in (65, 200):                                                         # the sort beyond one wavefront: descending ranges, some equal, some splitting
        spans, groups, ranges = [], [], []
        for g in range(ng):
            f = 1 + 4 * g
            spans += [(f, f + 1), (f + 3, f + 3)] if g % 7 == 0 else [(f, f + 3)]
        r = 0
        for g in range(ng):
            k = 2 if g % 7 == 0 else 1
            groups.append(list(range(r, r + k))); r += k
            ranges.append((4 * ng - 4 * (g // 3), 4 * ng + 8) if g % 7 else (1 + 4 * g, 4 + 4 * g))
        C[f"groups_{ng}"] = (spans, groups, ranges)
    return C


def random_contig(seed, max_reads=200):
    """A sparse short-read contig: (spans in Frag::cmp order, groups, ranges).  Blocks of SNPs, two groups per block; a read sits in the groups of the block its
    first SNP lies in — in one of them, or (one read in four) in both, so the re-insertion has a choice.  Coverage is thin: gaps inside a group's range are common."""
    rng = np.random.default_rng([20261019, seed])
    n_reads = int(rng.integers(4, max_reads + 1))
    n_snps = int(rng.integers(n_reads, 3 * n_reads + 8))
    f = np.sort(rng.integers(1, n_snps + 1, n_reads))
    l = np.minimum(f + rng.integers(0, 4, n_reads), n_snps)
    order = np.lexsort((np.arange(n_reads), -l, f))
    spans = [(int(f[i]), int(l[i])) for i in order]
    blk = int(rng.integers(20, 80))
    n_blk = (n_snps + blk - 1) // blk
    groups = [[] for _ in range(2 * n_blk)]
    ranges = []
    for b in range(n_blk):
        ranges += [(1 + b * blk, min(n_snps, (b + 1) * blk))] * 2
    for r, (a, _) in enumerate(spans):
        b = (a - 1) // blk
        u = rng.random()
        if u < 0.75:
            groups[2 * b + int(rng.integers(0, 2))].append(r)
        else:
            groups[2 * b].append(r); groups[2 * b + 1].append(r)
    return spans, groups, ranges
