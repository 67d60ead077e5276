"""The numpy model of the -e / -l estimate (EpsilonEstimator of host/ingest.cpp, file_reader.rs:749-826; floria_hip_blob_estimate), written on pileup COLUMNS: it
visits the covered positions of every group in order and asks every record for its base there, as the function is stated, not as the kernels split it.

A record is (pos, cigar, codes): cigar a list of (op, len), codes the 4-bit base codes (len(codes) is l_seq).  Records are already filtered (mapped, no 1796 flag,
at least one operation) and ascend by pos inside a group."""
import numpy as np

PERIOD, DEEP = 1000, 5
REF_OPS, QUERY_OPS, BASE_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8), (0, 7, 8)


def span_end(pos, cigar):
    n = sum(ln for op, ln in cigar if op in REF_OPS)
    return pos + (n if n else 1)


_TABLES = {}


def _tables(cigar):
    """per operation: (op, reference offset in front of it, reference offset behind it, query offset in front of it); kept per CIGAR list, a long one is asked often"""
    t = _TABLES.get(id(cigar))
    if t is None or t[0] is not cigar:
        op = np.array([o for o, _ in cigar], np.int64); ln = np.array([n for _, n in cigar], np.int64)
        r_end = np.cumsum(np.where(np.isin(op, REF_OPS), ln, 0)); q_end = np.cumsum(np.where(np.isin(op, QUERY_OPS), ln, 0))
        t = _TABLES[id(cigar)] = (cigar, op, r_end - np.where(np.isin(op, REF_OPS), ln, 0), r_end, q_end - np.where(np.isin(op, QUERY_OPS), ln, 0))
    return t[1:]


def base_at(rec, p):
    """the code the record gives at reference position p: that of the first reference-consuming operation that ends behind p, if it is M, = or X and its query
    offset there is below l_seq; None for a deletion, a refskip, a query offset at or beyond l_seq, or no operation there"""
    pos, cigar, codes = rec
    op, r_begin, r_end, q_begin = _tables(cigar)
    k = int(np.searchsorted(r_end, p - pos, side="right"))
    if p < pos or k == len(op) or op[k] not in BASE_OPS:
        return None
    sp = int(q_begin[k] + (p - pos - r_begin[k]))
    return int(codes[sp]) if sp < len(codes) else None


def estimate(groups, stop=1000, count=0, n_err=0):
    """groups: a list of lists of records -> dict(cols = [(group, pos, total, most)] of every sampled column in order, rec_hits (one per record, the groups
    concatenated), count, n_err, done)"""
    cols, hits = [], [np.zeros(len(g), np.int64) for g in groups]
    done = n_err >= stop
    for gi, recs in enumerate(groups):
        if done or not recs:
            continue
        starts = np.array([r[0] for r in recs], np.int64)
        ends = np.array([span_end(r[0], r[1]) for r in recs], np.int64)
        lo, hi = int(starts.min()), int(ends.max())
        diff = np.zeros(hi - lo + 1, np.int64)
        np.add.at(diff, starts - lo, 1); np.add.at(diff, ends - lo, -1)
        columns = np.flatnonzero(np.cumsum(diff)[:-1] > 0) + lo
        j = 0
        while j < len(columns):
            if count % PERIOD:
                step = min(PERIOD - count % PERIOD, len(columns) - j)      # columns that only advance the count
                count += step; j += step
                continue
            p = int(columns[j]); j += 1
            by_code = np.zeros(16, np.int64)
            for i in np.flatnonzero((starts <= p) & (ends > p)):
                b = base_at(recs[i], p)
                if b is not None:
                    by_code[b] += 1; hits[gi][i] += 1
            total, most = int(by_code.sum()), int(by_code.max())
            cols.append((gi, p, total, most))
            if total < DEEP:
                continue
            n_err += 1
            if n_err >= stop:
                done = True
                break
            count += 1
    return dict(cols=cols, rec_hits=np.concatenate(hits) if hits else np.zeros(0, np.int64), count=count, n_err=n_err, done=done)


def result(cols, lengths):
    """(-l, -e) from the sampled columns and the multiset of lengths [(l_seq, multiplicity)]: EpsilonEstimator::result"""
    lens = sorted(l for l, m in lengths for _ in range(int(m)))
    if not lens:
        return 500, 0.01
    errs = sorted((t - m) / m for _, _, t, m in cols if t >= DEEP)
    return max(lens[len(lens) * 66 // 100], 500), max(errs[len(errs) * 66 // 100] if errs else 0.0, 0.01)


def lengths_of(groups, rec_hits):
    """the sorted (l_seq, multiplicity) pairs of the length multiset"""
    d = {}
    for rec, h in zip([r for g in groups for r in g], rec_hits):
        if h:
            d[len(rec[2])] = d.get(len(rec[2]), 0) + int(h)
    return sorted(d.items())
