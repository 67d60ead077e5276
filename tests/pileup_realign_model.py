"""Model of floria_hip_pileup_records_realign and of floria-hip --pileup fused: alignment::realign (alignment.rs:7-64) applied to the cells of
tests/pileup_model.py: walk_records, written from the reference's formulation and the conventions of the C header, not from the product:

  * a cell is looked at only when 16 <= G, G + 16 < R, 16 <= p and p + 16 < L (G the SNP's genome position, R the length of the contig's reference
    sequence, p the cell's seq_pos with the hard-clip shift, L the record's l_seq); a contig without a reference has R = 0;
  * the read window is the record's own bases p - 16 .. p + 15 with everything but A C G T turned into A (DnaString::from_acgt_bytes), the
    reference window the upper-cased reference bytes G - 16 .. G + 15, the candidates the site's alleles upper-cased;
  * every candidate is scored with the candidate in column 16 of the reference window and the FIRST best one wins (`score > best_score`).  The exact
    shortcut the issue describes (h mismatches outside column 16) is no rule of its own here: the model scores every in-bounds cell with
    realign_walk_model.exact_scores / model_scores and only REPORTS which cells the shortcut would decide — the tests assert that the two agree.

Also here: the crafted case (every boundary of the rule) and the seeded sweep (noisy reads cut from a reference) the CPU and GPU tests share."""
import numpy as np

from tests import pileup_model as pm
from tests import realign_walk_model as wm

FL = 16
_ACGT = np.zeros(256, bool)
_ACGT[list(b"ACGT")] = True
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32


def upper(a):
    return _UPPER[np.asarray(a, np.uint8)]


def realign_records(records, tables, refs, member=None, walked=None, lo=FL, hi=FL, unshifted=False, keep_n=False, last_best=False, use_shortcut=False):
    """records / tables as pileup_model.walk_records takes them, refs: one bytes object per table (b"" = no reference) -> (result, counts, detail):
    result = the six arrays of walk_records with the realigned alleles, counts = dict(cells, in_bounds, shortcut, scored, changed), detail = per-cell
    arrays (record, k, G, p, L, R, in_bounds, h, has, undecided, decided, n_alleles, non_acgt, lower_ref, q16, walked_base, walked_allele) for the assertions on the fixtures.
    member: None = the exact DP, (step, rule, tie) = that fixed-block walk.
    The keyword arguments after `walked` make WRONG models: lo / hi move the two bounds (the rule is lo <= x and x + hi < len), unshifted takes p without
    the hard-clip shift, keep_n leaves non-ACGT read bases as they are, last_best lets a later equal score win.  use_shortcut=True decides the shortcut's
    cells by the shortcut instead of by scoring (same result; the sweep uses it to save time, one test shows the equality)."""
    walked = pm.walk_records(records, tables) if walked is None else walked
    cell_off, snp, allele, qual, seq_pos, ref_end = walked
    n = int(cell_off[-1])
    rec_of = np.repeat(np.arange(len(records)), np.diff(cell_off).astype(np.int64))
    d = dict(record=rec_of, k=snp.astype(np.int64) - 1, G=np.zeros(n, np.int64), p=seq_pos.astype(np.int64), L=np.zeros(n, np.int64), R=np.zeros(n, np.int64),
             in_bounds=np.zeros(n, bool), h=np.full(n, -1, np.int64), has=np.zeros(n, bool), undecided=np.zeros(n, bool), n_alleles=np.zeros(n, np.int64),
             non_acgt=np.zeros(n, bool), lower_ref=np.zeros(n, bool), q16=np.zeros(n, np.uint8), walked_base=np.zeros(n, np.uint8))
    Q = np.full((n, 2 * FL), ord("A"), np.uint8); Rw = np.full((n, 2 * FL), ord("A"), np.uint8)
    AL = np.zeros((n, 4), np.uint8)
    pad = 2 * FL + 2                                                      # (the wrong models with looser bounds read up to two bytes outside: those are 'A')
    ref_pad = [np.concatenate([np.full(pad, ord("A"), np.uint8), np.frombuffer(bytes(r), np.uint8), np.full(pad, ord("A"), np.uint8)]) for r in refs]
    cols = np.arange(2 * FL) - FL
    for i, rec in enumerate(records):
        a, b = int(cell_off[i]), int(cell_off[i + 1])
        if a == b:
            continue
        t = tables[rec["contig"]]
        seq = np.frombuffer(rec["seq"], np.uint8)
        hard = int(rec["cigar"][0][1]) if (rec["flag"] & 0x800) and rec["cigar"] and rec["cigar"][0][0] == "H" else 0
        k = d["k"][a:b]
        G = t.pos[k]
        p = d["p"][a:b]
        d["walked_base"][a:b] = seq[(p - hard) & 0xffffffff]
        if unshifted:
            p = (p - hard) & 0xffffffff
        L, R = len(seq), len(refs[rec["contig"]])
        d["G"][a:b] = G; d["L"][a:b] = L; d["R"][a:b] = R; d["n_alleles"][a:b] = t.n_alleles[k]
        AL[a:b] = upper(t.alleles[k])
        ok = (lo <= G) & (G + hi < R) & (lo <= p) & (p + hi < L)
        d["in_bounds"][a:b] = ok
        if not ok.any():
            continue
        sp = np.concatenate([np.full(pad, ord("A"), np.uint8), seq, np.full(pad, ord("A"), np.uint8)])
        qi = p[ok, None] + cols[None, :] + pad
        q = sp[qi]
        d["non_acgt"][a:b][ok] = (~_ACGT[q]).any(axis=1)
        if not keep_n:
            q = np.where(_ACGT[q], q, ord("A")).astype(np.uint8)
        r = ref_pad[rec["contig"]][G[ok, None] + cols[None, :] + pad]
        d["lower_ref"][a:b][ok] = (r != upper(r)).any(axis=1)
        Q[a:b][ok] = q; Rw[a:b][ok] = upper(r)
    inb = d["in_bounds"]
    mism = Q != Rw
    mism[:, FL] = False
    h = mism.sum(axis=1)
    d["h"][inb] = h[inb]
    d["q16"][:] = Q[:, FL]
    na = d["n_alleles"]
    eq = (AL == Q[:, FL:FL + 1]) & (np.arange(4)[None, :] < na[:, None])
    d["has"][:] = eq.any(axis=1) & inb
    first_eq = np.argmax(eq, axis=1)
    by_base = inb & (h <= 2) & d["has"]
    by_first = inb & ~by_base & (h <= 1)
    d["undecided"][:] = inb & ~by_base & ~by_first
    out = allele.copy()
    score_these = d["undecided"] if use_shortcut else inb
    if use_shortcut:
        out[by_base] = first_eq[by_base]; out[by_first] = 0
    idx = np.nonzero(score_these)[0]
    if len(idx):
        scores = np.full((4, len(idx)), np.iinfo(np.int32).min, np.int64)
        for m in range(4):
            sel = np.nonzero(na[idx] > m)[0]
            if len(sel):
                Rm = Rw[idx[sel]].copy(); Rm[:, FL] = AL[idx[sel], m]
                scores[m, sel] = wm.exact_scores(Q[idx[sel]], Rm) if member is None else wm.model_scores(Q[idx[sel]], Rm, member)
        best = (3 - np.argmax(scores[::-1], axis=0)) if last_best else wm.first_best(scores)[0]
        out[idx] = best
    counts = dict(cells=n, in_bounds=int(inb.sum()), shortcut=int((by_base | by_first).sum()), scored=int(d["undecided"].sum()), changed=int((out != allele).sum()))
    d["shortcut_allele"] = np.where(by_base, first_eq, 0)
    d["decided"] = by_base | by_first
    d["walked_allele"] = allele
    return (cell_off, snp, out.astype(np.uint8), qual, seq_pos, ref_end), counts, d


def pack_refs(refs):
    """list of bytes -> ref_off uint64 [n + 1], ref_seq uint8"""
    off = np.zeros(len(refs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in refs])
    return off, np.frombuffer(b"".join(bytes(r) for r in refs), np.uint8)


def subset(records, order):
    return [records[i] for i in order]


def pick_records(per_record, total, need=None, zeros=6):
    """ascending indices of records whose per_record numbers add up to exactly `total`, taken greedily, plus up to `zeros` records whose number is 0
    (with `need`: only those it marks)"""
    order, left = [], int(total)
    for i, c in enumerate(per_record):
        c = int(c)
        if c == 0:
            if zeros and (need is None or need[i]):
                order.append(i); zeros -= 1
        elif c <= left:
            order.append(i); left -= c
    assert left == 0, (total, left)
    return order


# ---- the crafted case ------------------------------------------------------------------------------------------------------------------------------
_BASES = np.frombuffer(b"ACGT", np.uint8)


def _site_tables(rng, ref, sites):
    """REF = the upper-cased reference base, then the other three bases in a random order; 1, 2, 3, 4, 1, .. alleles"""
    al = np.zeros((len(sites), 4), np.uint8); na = np.zeros(len(sites), np.uint8)
    for x, g in enumerate(sites):
        ref_b = int(upper(ref[g:g + 1])[0]) if _ACGT[int(upper(ref[g:g + 1])[0])] else ord("A")
        others = [int(b) for b in _BASES if b != ref_b]
        order = rng.permutation(3)
        na[x] = x % 4 + 1
        full = [ref_b] + [others[o] for o in order]
        al[x, :na[x]] = full[:na[x]]
    return pm.SnpTable(np.asarray(sites, np.int64), al, na)


def crafted_case():
    """-> (records, tables, refs).  Three contigs: 0 and 1 with reference sequences of odd and even length (lower-case stretches, an N), 2 without one.
    Most records are supplementary alignments with a leading hard clip, built so that the SHIFTED seq_pos lands where the case needs it: at 15, 16,
    L - 17, L - 16, with the SNP at G = 15, 16, R - 17, R - 16, over windows with 0..3 mismatches whose centre is another allele, the walked allele, no
    allele at all or an N.  Plain records (M / I / D / S) with noise complete it."""
    rng = np.random.default_rng(20260311)
    R0, R1 = 333, 410
    refs = []
    for R in (R0, R1):
        r = _BASES[rng.integers(0, 4, size=R)].copy()
        r[90:115] += 32; r[R - 40:R - 20] += 32                            # lower case
        r[205] = ord("N"); r[150] = ord("n")
        refs.append(r.tobytes())
    refs.append(b"")
    sites0 = [15, 16, 70, 100, 101, 130, 160, 200, 240, 270, R0 - 17, R0 - 16]
    sites1 = [15, 16, 50, 99, 148, 202, 260, 300, 340, R1 - 17, R1 - 16]
    refn = [np.frombuffer(r, np.uint8) for r in refs]
    tables = [_site_tables(rng, refn[0], sites0), _site_tables(rng, refn[1], sites1),
              pm.SnpTable([20, 40, 60], [[65, 67, 0, 0]] * 3, [2, 2, 2])]
    recs = []

    def add(contig, pos, cigar, seq, flag=0):
        recs.append(pm.make_record(pos, cigar, bytes(seq), rng.integers(0, 60, size=len(seq)).astype(np.uint8), flag=flag, contig=contig,
                                   name="k%d" % len(recs) + "y" * (len(recs) % 3)))

    def probe(contig, k, p, L, h, centre, sp=None, walked=None):
        """supplementary record H<p - sp> M<L> whose base sp sits on SNP k (so the walk calls it there) and whose shifted seq_pos is p: bases p - 16 .. p + 15
        are the reference window of the SNP with h columns changed and `centre` in the middle"""
        t, ref = tables[contig], refn[contig]
        G, na = int(t.pos[k]), int(t.n_alleles[k])
        sp = min(5, G, p - 1) if sp is None else sp
        hard = p - sp
        seq = _BASES[rng.integers(0, 4, size=L)].copy()
        inside = [j for j in range(2 * FL) if 0 <= p - FL + j < L and 0 <= G - FL + j < len(ref)]
        for j in inside:
            b = int(upper(ref[G - FL + j:G - FL + j + 1])[0])
            seq[p - FL + j] = b if _ACGT[b] else ord("A")
        for j in rng.permutation([j for j in inside if j != FL and p - FL + j != sp])[:h]:
            seq[p - FL + j] = _BASES[(int(np.searchsorted(_BASES, seq[p - FL + j])) + 1 + int(rng.integers(0, 3))) % 4]
        w = int(rng.integers(0, na)) if walked is None else walked
        alle = [int(x) for x in t.alleles[k, :na]]
        if 0 <= p < L:
            if centre == "other":
                seq[p] = alle[(w + 1) % na]
            elif centre == "same":
                seq[p] = alle[w]
            elif centre == "none":
                seq[p] = [int(b) for b in _BASES if int(b) not in alle][0]
            elif centre == "N":
                seq[p] = ord("N")
        seq[sp] = alle[w]
        add(contig, G - sp, [("H", hard), ("M", L)], seq, flag=0x800)

    # the bounds on p: SNPs in the middle of the contig (k = 3..8 of contig 0: 1 to 4 alleles), L = 120
    for contig in (0, 1):
        for k in (3, 4, 5, 6, 7):
            for p, L in ((15, 120), (16, 120), (60, 77), (60, 76), (103, 120), (104, 120)):
                probe(contig, k, p, L, 0, "other")
    # the bounds on G: the first two and the last two SNPs, p in the middle
    for contig in (0, 1):
        n_s = len(tables[contig].pos)
        for k in (0, 1, n_s - 2, n_s - 1):
            for centre in ("other", "same", "none"):
                if not ((centre == "other" and tables[contig].n_alleles[k] < 2) or (centre == "none" and tables[contig].n_alleles[k] > 3)):
                    probe(contig, k, 60, 120, 0, centre)
    # h = 0..3 (and more) x centre kinds x 1..4 alleles, odd and even p
    for contig in (0, 1):
        for k in range(2, 9):
            for h in (0, 1, 2, 3, 4, 7):
                for centre in ("other", "same", "none", "N"):
                    if (centre == "other" and tables[contig].n_alleles[k] < 2) or (centre == "none" and tables[contig].n_alleles[k] > 3):
                        continue
                    probe(contig, k, 60 + (h + k) % 2, 121, h, centre, sp=int(rng.integers(0, 30)))
    # the same kind of record on the contig without a reference
    probe(2, 1, 60, 120, 0, "other")
    # plain records: the reference with substitutions, N bases, an insertion, a deletion, soft clips; one without any cell
    for contig in (0, 1):
        ref = refn[contig]
        for start, ln in ((0, 140), (1, 141), (55, 200), (120, len(ref) - 120), (180, 150), (60, 33), (61, 32)):
            s = upper(ref[start:start + ln]).copy()
            s[~_ACGT[s]] = ord("A")
            hit = rng.random(ln) < 0.12
            s[hit] = _BASES[rng.integers(0, 4, size=int(hit.sum()))]
            s[rng.random(ln) < 0.02] = ord("N")
            add(contig, start, [("M", ln)], s)
        s = upper(ref[40:240]).copy(); s[~_ACGT[s]] = ord("C")
        add(contig, 40, [("S", 4), ("M", 80), ("I", 3), ("M", 50), ("D", 6), ("M", 57), ("S", 6)],
            np.concatenate([s[:4], s[0:80], _BASES[[0, 1, 2]], s[80:130], s[136:193], s[:6]]))
        add(contig, 20, [("M", 30)], upper(ref[20:50]))                        # no SNP between 20 and 50: no cell
    add(2, 10, [("M", 80)], _BASES[rng.integers(0, 2, size=80) * 1])           # cells on the contig without a reference
    return recs, tables, refs


def sweep_case(seed=4242, n_records=320, sub_rate=0.05, hidden_indel=0.2, supp=0.1):
    """-> (records, tables, refs): reads of 60-260 bases cut from three reference sequences (the third one's SNP table is dense), with substitutions at
    sub_rate, N bases, CIGARs with I / D / S, supplementary records with hard clips, and — in a share of the reads — an insertion or deletion the CIGAR
    does not show, which is what realignment exists for: behind it the walk reads the neighbouring base."""
    rng = np.random.default_rng(seed)
    refs, tables = [], []
    for R, gap in ((3001, 9), (2200, 14), (1500, 5)):
        r = _BASES[rng.integers(0, 4, size=R)].copy()
        low = rng.random(R) < 0.1
        r[low] += 32
        refs.append(r.tobytes())
        pos = np.unique(np.clip(np.cumsum(rng.integers(1, 2 * gap, size=R // gap)), 0, R - 1))
        tables.append(_site_tables(rng, r, [int(x) for x in pos]))
    recs = []
    for i in range(n_records):
        c = int(rng.integers(0, 3))
        ref = np.frombuffer(refs[c], np.uint8)
        ln = int(rng.integers(60, 260))
        start = int(rng.integers(0, len(ref) - 40))
        ln = min(ln, len(ref) - start)
        s = upper(ref[start:start + ln]).copy()
        t = tables[c]
        inside = t.pos[(t.pos >= start) & (t.pos < start + ln)]
        for g in inside:                                                        # the read carries one of the site's alleles
            k = int(np.searchsorted(t.pos, g))
            s[g - start] = t.alleles[k, rng.integers(0, t.n_alleles[k])]
        hit = rng.random(ln) < sub_rate
        s[hit] = _BASES[rng.integers(0, 4, size=int(hit.sum()))]
        s[rng.random(ln) < 0.01] = ord("N")
        cigar = [("M", ln)]
        kind = rng.random()
        if kind < 0.15 and ln > 40:                                             # an insertion the CIGAR shows
            at, k = int(rng.integers(10, ln - 10)), int(rng.integers(1, 4))
            s = np.concatenate([s[:at], _BASES[rng.integers(0, 4, size=k)], s[at:]])
            cigar = [("M", at), ("I", k), ("M", ln - at)]
        elif kind < 0.3 and ln > 40:                                            # a deletion the CIGAR shows
            at, k = int(rng.integers(10, ln - 20)), int(rng.integers(1, 4))
            s = np.concatenate([s[:at], s[at + k:]])
            cigar = [("M", at), ("D", k), ("M", ln - at - k)]
        if rng.random() < hidden_indel and len(s) > 40:                         # ... and one it does not
            at = int(rng.integers(5, len(s) - 5))
            if rng.random() < 0.5:
                s = np.concatenate([s[:at], _BASES[rng.integers(0, 4, size=1)], s[at:-1]])
            else:
                s = np.concatenate([s[:at], s[at + 1:], _BASES[rng.integers(0, 4, size=1)]])
        flag = int(rng.choice([0, 16, 1 | 64, 1 | 128]))
        if rng.random() < 0.1:
            k = int(rng.integers(1, 9))
            s = np.concatenate([_BASES[rng.integers(0, 4, size=k)], s]); cigar = [("S", k)] + cigar
        if rng.random() < supp:
            flag = 0x800 | (16 if rng.random() < 0.5 else 0)
            cigar = [("H", int(rng.integers(1, 60)))] + cigar
        recs.append(pm.make_record(start, cigar, s.tobytes(), rng.integers(0, 94, size=len(s)).astype(np.uint8), flag=flag, contig=c, name="s%d" % i))
    return recs, tables, refs


_cache = {}


def cached(name, member=None):
    """('crafted' | 'sweep', member) -> (records, tables, refs, walked, (result, counts, detail)), computed once per process"""
    if name not in _cache:
        recs, tables, refs = crafted_case() if name == "crafted" else sweep_case()
        _cache[name] = (recs, tables, refs, pm.walk_records(recs, tables))
    key = (name, member)
    if key not in _cache:
        recs, tables, refs, walked = _cache[name]
        _cache[key] = realign_records(recs, tables, refs, member=member, walked=walked, use_shortcut=(name == "sweep"))
    return _cache[name] + (_cache[key],)
