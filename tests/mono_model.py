"""remove_monomorphic_allele (utils_frags.rs:713-772, --ignore-monomorphic) restated in numpy over Pileups: the model floria_hip_drop_monomorphic is tested
against (tests/test_mono_cpu.py pins it against the C++ host's own restatement, tests/test_gpu_mono.py compares the device with it).

    1. allele_count_map[snp][allele] += phred_scale(qual) over all reads' cells (f64 sums of f32 values that are multiples of 2^-24: exact in any order);
    2. a SNP of the map with one allele, or with vals[0] * error > vals[1] for its two largest sums, is removed from every read;
    3. reads left without cells are dropped; 4. the rest are sorted by Frag::cmp (with the old counter_id); 5. and renumbered.
"""
import ctypes as C
import ctypes.util

import numpy as np

from floria_amd.pileup import Pileup


def _weights():
    """utils_frags.rs:702-711 for every quality byte: 1f32 - 10f32.powf(-q / 10) with the C library's powf (numpy's float32 power rounds q = 2 the other way)"""
    powf = C.CDLL(ctypes.util.find_library("m")).powf
    powf.restype, powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return np.array([np.float32(1.0) - np.float32(powf(10.0, float(np.float32(q) / np.float32(-10.0)))) for q in range(256)], np.float32).astype(np.float64)


WEIGHT = _weights()


def phred_scale(qual):
    """the weights of quality bytes, widened to f64 as the reference widens them"""
    return WEIGHT[np.asarray(qual).astype(np.int64)]


def removed_mask(p: Pileup, n_snps, error):
    """uint8 [n_snps]: 1 where SNP s = index + 1 is removed"""
    w = np.zeros((n_snps, 4), np.float64)
    key = np.zeros((n_snps, 4), bool)
    s = p.snp.astype(np.int64) - 1
    np.add.at(w, (s, p.allele.astype(np.int64)), phred_scale(p.qual))
    key[s, p.allele.astype(np.int64)] = True
    out = np.zeros(n_snps, np.uint8)
    for i in np.nonzero(key.any(axis=1))[0]:                    # the SNPs the map has
        vals = sorted((float(w[i, a]) for a in range(4) if key[i, a]), reverse=True)
        out[i] = 1 if len(vals) == 1 or vals[0] * error > vals[1] else 0
    return out


def drop_monomorphic(p: Pileup, n_snps, error):
    """-> (filtered Pileup, old_read uint32 [reads of the result], removed uint8 [n_snps])"""
    removed = removed_mask(p, n_snps, error)
    keep = removed[p.snp.astype(np.int64) - 1] == 0 if p.n_cells else np.zeros(0, bool)
    reads = []
    for r in range(p.n_reads):
        lo, hi = int(p.read_off[r]), int(p.read_off[r + 1])
        k = keep[lo:hi]
        if k.any():
            reads.append((r, p.snp[lo:hi][k], p.allele[lo:hi][k], p.qual[lo:hi][k]))
    reads.sort(key=lambda x: (int(x[1][0]), -int(x[1][-1]), x[0]))      # Frag::cmp, counter_id = the old index
    off = np.zeros(len(reads) + 1, np.uint32)
    off[1:] = np.cumsum([len(x[1]) for x in reads])
    cat = (lambda i, dt: np.concatenate([x[i] for x in reads]).astype(dt) if reads else np.zeros(0, dt))
    q = Pileup(off, cat(1, np.uint32), cat(2, np.uint8), cat(3, np.uint8), np.array([x[1][0] for x in reads], np.uint32), np.array([x[1][-1] for x in reads], np.uint32))
    return q, np.array([x[0] for x in reads], np.uint32), removed


def drop_batch(pileups, snp_counts, error):
    """the model of one floria_hip_drop_monomorphic call -> (filtered pileups, dict as FloriaHip.drop_monomorphic returns it)"""
    outs = [drop_monomorphic(p, n, error) for p, n in zip(pileups, snp_counts)]
    read_off = np.zeros(len(pileups) + 1, np.uint64)
    read_off[1:] = np.cumsum([o[0].n_reads for o in outs])
    removed = np.concatenate([o[2] for o in outs] + [np.zeros(0, np.uint8)])
    res = dict(read_off=read_off, old_read=np.concatenate([o[1] for o in outs] + [np.zeros(0, np.uint32)]).astype(np.uint32), removed=removed,
               n_removed_snps=int(removed.sum()), n_removed_cells=sum(p.n_cells for p in pileups) - sum(o[0].n_cells for o in outs),
               n_dropped_reads=sum(p.n_reads for p in pileups) - sum(o[0].n_reads for o in outs))
    return [o[0] for o in outs], res


def filter_set_order(old_snps, old_order, removed):
    """a read's set_order after the removals: the old iteration order with the removed cells deleted (a `remove` moves no other key), the rest renumbered"""
    old_snps = np.asarray(old_snps, np.int64)
    keep = removed[old_snps - 1] == 0
    new_index = np.cumsum(keep) - 1
    order = np.asarray(old_order, np.int64)
    return new_index[order[keep[order]]].astype(np.uint32)


# ---- the hand case: one site of every rule, at error = 0.5 -------------------------------------------------------------------------------------------------
# phred_scale(10) = 0.9f32 =: w.  SNP 1: one allele -> removed.  SNP 2: allele 0 twice at q 10, allele 1 once at q 10: 2w * 0.5 == w exactly -> kept.
# SNP 3: allele 1 once at q 9 instead (0.874.. < w) -> removed.  SNP 4: the minor allele only at q 0: two keys, 0 < v0 * 0.5 -> removed.  SNP 5: three alleles
# (4 : 3 : 1 reads at q 30) -> kept.  SNP 6 and 9: nobody calls them -> not in the map, not removed.  SNP 7 (4 : 2, equality again) and 8 (3 : 2) -> kept.
HAND_ERROR = 0.5
HAND_SNPS = 9
HAND_MASK = np.array([1, 0, 1, 1, 0, 0, 0, 0, 0], np.uint8)
HAND_READS = [
    {1: (0, 30), 2: (0, 10), 3: (0, 10), 4: (0, 20), 5: (0, 30)},
    {1: (0, 30), 2: (0, 10), 3: (0, 10), 4: (0, 20), 5: (1, 30), 7: (0, 30), 8: (1, 30)},
    {1: (0, 25), 3: (1, 9)},                                    # every cell at a removed SNP: the read is dropped
    {1: (0, 30), 2: (1, 10), 4: (1, 0), 5: (2, 30), 7: (1, 30)},
    {4: (0, 20), 5: (0, 30), 7: (0, 30)},                       # first 4 -> 5: now behind the next read, which ends later
    {5: (1, 30), 7: (1, 30), 8: (0, 30)},
    {5: (0, 30), 7: (0, 30), 8: (1, 30)},                       # (5, 8) like the one before: the old index decides
    {1: (0, 30), 5: (0, 30), 8: (0, 30)},                       # first 1 -> 5
    {4: (0, 20), 5: (1, 30), 8: (1, 30)},                       # first 4 -> 5
    {7: (0, 30)},
]


def hand_pileup():
    return Pileup.from_reads([(sorted(r), [r[s][0] for s in sorted(r)], [r[s][1] for s in sorted(r)]) for r in HAND_READS])
