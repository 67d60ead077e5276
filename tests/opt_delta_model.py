"""numpy / Python restatement of the optimise rounds of one (block, ploidy) job in the canonical arithmetic, as optimize_kernel.h runs them (local_clustering.rs:71-130,
292-358): histogram of (read count, Q24 sum) per (position, partition, allele), one code byte per (position, partition), distances as exact packed integers
(diff Q24 << 16 | #empty), candidates sorted by (gain desc, partition, read, target), the serial application, accept / undo.

What it is for ("opt_delta"):
  * behind every accepted round it forms the next round's distances twice — by exchanging term(old code) for term(new code) at the cells that sit on a flipped
    (position, partition) pair, found with find_cell (the kernel's search, restated), and by a full recomputation — and asserts that they are the same integers;
  * it reports, per round, the flips and which pass the kernel takes (delta / interval / none), so a GPU test can pick inputs that reach the path it names and
    predict the library's optimize_delta_passes / optimize_delta_fallbacks counters.
It is pinned to the oracle (tests/test_opt_delta_cpu.py): same optimised partition and round count as oracle.one_ploidy."""
import struct

import numpy as np

ONE_Q24 = 1 << 24
NUM_ITER_OPTIMIZE = 20
FLIP_CAP = 64          # optimize_kernel.h: OPT_FLIP_CAP
DELTA_DIV = 4          # optimize_kernel.h: OPT_DELTA_DIV


def find_cell(deltas, d):
    """index of the cell at delta d in the strictly ascending `deltas` (deltas[j] >= j), or -1; returns (index, probes).  optimize_kernel.h: opt_find_cell."""
    n = len(deltas)
    lo, hi, step = 0, min(d, n - 1), 0
    probes = []
    while lo <= hi:
        j = hi if step == 0 else (lo if step == 1 else (lo + hi) >> 1)
        assert 0 <= j < n
        probes.append(j)
        dj = int(deltas[j])
        if dj == d:
            return j, probes
        b = d - (dj - j)
        if dj > d:
            hi, lo = j - 1, max(lo, b)
        else:
            lo, hi = j + 1, min(hi, b)
        step += 1
    return -1, probes


def _f64(t, eps):
    return float(t >> 16) * 2.0 ** -24 + float(t & 0xffff) * eps          # qm_to_f64: multiply and add round separately


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _term(c, al, w):
    return 1 if c == 0 else (0 if (c >> al) & 1 else w << 16)


class Job:
    def __init__(self, pileup, read_ids, part, ploidy, eps, w24, alleles=2):
        self.p, self.eps, self.A = ploidy, eps, alleles
        self.reads = []
        for r in read_ids:
            s, a, q = pileup.read(int(r))
            self.reads.append((s.astype(np.int64), a.astype(np.int64), np.asarray(w24, np.int64)[q]))
        self.pos0 = min(int(s[0]) for s, _, _ in self.reads)
        self.span = max(int(s[-1]) for s, _, _ in self.reads) - self.pos0 + 1
        self.part = [int(k) for k in part]
        self.cnt = np.zeros((self.span, ploidy, alleles), np.int64)
        self.q = np.zeros((self.span, ploidy, alleles), np.int64)
        for i, k in enumerate(self.part):
            self._add(i, k, 1)
        self.size = [self.part.count(k) for k in range(ploidy)]

    def _add(self, i, k, sign):
        s, a, w = self.reads[i]
        np.add.at(self.cnt, (s - self.pos0, k, a), sign)
        np.add.at(self.q, (s - self.pos0, k, a), sign * w)

    def codes(self):
        mx = self.q.max(axis=2)
        c = np.zeros((self.span, self.p), np.int64)
        for a in range(self.A):
            c |= ((mx != 0) & (self.q[:, :, a] == mx)).astype(np.int64) << a
        return c

    def score(self):
        s = 0.0
        for k in range(self.p):
            have = self.cnt[:, k, :].sum(axis=1) > 0
            mx = self.q[:, k, :].max(axis=1)
            eq = int((self.q[:, k, :].sum(axis=1) - mx)[have].sum())
            em = int((have & (mx <= ONE_Q24)).sum())
            s += float(eq) * 2.0 ** -24 + float(em) * self.eps
        return s * -1.0

    def distances(self, codes):
        t = [[0] * self.p for _ in self.reads]
        for i, (s, a, w) in enumerate(self.reads):
            for x in range(len(s)):
                for k in range(self.p):
                    t[i][k] += _term(int(codes[int(s[x]) - self.pos0, k]), int(a[x]), int(w[x]))
        return t

    def delta_update(self, t, flips, limit=None):
        """the delta pass: exchange the terms at the flipped (position, partition) pairs; returns the number of cells found and what the pass met: "first" / "last" (a flip
        at a read's first / last position), "gap" (a read spans the position and has no cell there), "to0" / "from0" (a code byte that becomes / was 0: the #empty field),
        "two_same" / "two_diff" (two cells of one read exchanged in the same / in different partitions), "long" (a read of more than 256 cells), "bisect" (a search that
        took more than two probes).  limit: only the first `limit` reads are visited (run's delta_reads)"""
        found, met = 0, set()
        for i, (s, a, w) in enumerate(self.reads[:limit]):
            f0, l0 = int(s[0]) - self.pos0, int(s[-1]) - self.pos0
            hit = []
            for pr, k, co, cn in flips:
                if pr < f0 or pr > l0:
                    continue
                j, probes = find_cell(s - int(s[0]), pr - f0)
                if len(probes) > 2:
                    met.add("bisect")
                if j < 0:
                    met.add("gap")
                    continue
                found += 1
                hit.append(k)
                met |= {"first"} if j == 0 else set()
                met |= {"last"} if j == len(s) - 1 else set()
                met |= {"to0"} if cn == 0 else set()
                met |= {"from0"} if co == 0 else set()
                met |= {"long"} if len(s) > 256 else set()
                t[i][k] += _term(cn, int(a[j]), int(w[j])) - _term(co, int(a[j]), int(w[j]))
            if len(hit) > len(set(hit)):
                met.add("two_same")
            if len(set(hit)) > 1:
                met.add("two_diff")
        return found, met

    def pass_taken(self, flips):
        """'none' | 'delta' | 'interval': what the kernel does with this many flips (optimize_kernel.h: dmode)"""
        if not flips:
            return "none"
        if len(flips) > FLIP_CAP:
            return "interval"
        lo, hi = min(f[0] for f in flips), max(f[0] for f in flips)
        inside = [len(s) for s, _, _ in self.reads if not (int(s[-1]) - self.pos0 < lo or int(s[0]) - self.pos0 > hi)]
        return "delta" if len(flips) * len(inside) * DELTA_DIV <= sum(inside) else "interval"


def run(pileup, read_ids, part, ploidy, eps, w24, alleles=2, delta_reads=None):
    """-> (optimised partition, rounds run, [per round with moves: {"flips": [(position, partition, old, new)], "accepted": bool, "pass": what the NEXT round's distance
    pass is, "cells": cells the delta update touched, "met": the cases it met (Job.delta_update), "M": the round's candidate moves, "M2": the power of two the kernel
    sorts them in (optimize_kernel.h: in LDS up to OPT_SORT_LDS, in the global pools beyond)}])
    delta_reads (sensitivity checks only; None = the kernel): a BROKEN kernel whose delta pass visits only the first delta_reads reads of the block — behind a delta pass the
    other reads keep their stale distances, the interval pass stays whole.  A test that must notice such a kernel picks inputs on which this run leaves the oracle."""
    J = Job(pileup, read_ids, part, ploidy, eps, w24, alleles)
    n, p = len(J.reads), ploidy
    rounds, iters = [], 0
    prev = J.score()
    codes = J.codes()
    t = None
    for it in range(NUM_ITER_OPTIMIZE):
        iters = it + 1
        if p == 1:
            break
        if t is None:
            t = J.distances(codes)
        cand = []
        for i in range(n):
            pi = J.part[i]
            for j in range(p):
                if j == pi or J.size[pi] <= 1:
                    continue
                diff = _f64(t[i][pi], eps) - _f64(t[i][j], eps)
                if diff > 0.0:
                    cand.append((-_bits(diff), (pi << 28) | (i << 4) | j))
        if not cand:
            break
        cand.sort()
        M = len(cand)
        number = M // 10
        if number == 0:
            number = M // 3 + 1
        moved, moves = set(), []
        for mv, (_, key) in enumerate(cand):
            i, rl, j = key >> 28, (key >> 4) & 0xffffff, key & 15
            if rl in moved or J.size[i] == 1:
                continue
            J.size[j] += 1
            J.size[i] -= 1
            moved.add(rl)
            moves.append((rl, i, j))
            if mv > number:
                break
        for rl, i, j in moves:
            J._add(rl, i, -1)
            J._add(rl, j, 1)
            J.part[rl] = j
        new_codes = J.codes()
        flips = [(int(pr), int(k), int(codes[pr, k]), int(new_codes[pr, k])) for pr, k in zip(*np.nonzero(codes != new_codes))]
        new = J.score()
        M2 = 1
        while M2 < M:
            M2 <<= 1
        info = {"flips": flips, "accepted": new > prev, "pass": "none", "cells": 0, "met": set(), "M": M, "M2": M2}
        rounds.append(info)
        if new > prev:
            prev = new
            info["pass"] = J.pass_taken(flips) if it + 1 < NUM_ITER_OPTIMIZE else "none"          # (the pass opens the next round)
            info["cells"], info["met"] = J.delta_update(t, flips, delta_reads)
            full = J.distances(new_codes)
            if delta_reads is None:
                assert t == full, ("the per-position update differs from the full recomputation", it, flips)
            elif info["pass"] != "delta":
                t = full
            codes = new_codes
        else:
            for rl, i, j in moves:
                J._add(rl, j, -1)
                J._add(rl, i, 1)
                J.part[rl] = i
                J.size[i] += 1
                J.size[j] -= 1
            break
    return np.array(J.part, np.uint8), iters, rounds
