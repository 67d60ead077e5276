"""Model of one alignment record's SNP calls (frag_from_record, file_reader.rs:661-736) for the tests of floria_hip_pileup_records and
floria-hip --pileup, written from the reference's behaviour in ITS formulation: rust-htslib's aligned_pairs_full yields one
(query position | None, reference position | None) pair per base of every CIGAR operation (file_reader.rs:673-727), and a pair with both sides
present whose reference position is a SNP of the contig gives a call when the read base is one of the site's alleles.  Nothing here merges a
cursor through the SNP table the way the host walk (floria_amd/host/ingest.cpp) and the kernel (csrc/pileup_kernel.h) do: the pairs are
enumerated (with numpy, a record at a time) and looked up.

Also here: a record builder on top of floria_amd.synth_bam.bam_record for arbitrary CIGARs, the packing of such records into the blob + offset
arrays the C ABI takes, the crafted records and the seeded random generator the CPU and GPU tests share.
"""
import struct

import numpy as np

from floria_amd import synth_bam

NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
OPS = "MIDNSHP=X"
Q_OPS, R_OPS, PAIR_OPS = set("MIS=X"), set("MDN=X"), set("M=X")


class SnpTable:
    """positions [n] int64 ascending, alleles [n, 4] uint8 (REF then ALTs), n_alleles [n] uint8 of one contig"""

    def __init__(self, pos, alleles, n_alleles):
        self.pos = np.asarray(pos, np.int64)
        self.alleles = np.asarray(alleles, np.uint8).reshape(-1, 4)
        self.n_alleles = np.asarray(n_alleles, np.uint8)
        assert len(self.pos) == len(self.alleles) == len(self.n_alleles)


def aligned_pairs_full(pos, cigar):
    """(q [k], r [k], has_q [k], has_r [k]): one pair per base of every operation, in order (H and P yield none); has_* False = None on that side
    (a reference position of -1 is legal for a record at pos -1, so None is not told by value)"""
    qs, rs, hq, hr = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, bool)], [np.zeros(0, bool)]
    q, r = 0, int(pos)
    for op, ln in cigar:
        ln = int(ln)
        if op in PAIR_OPS or op in ("I", "S", "D", "N"):
            qs.append(np.arange(q, q + ln) if op in Q_OPS else np.zeros(ln, np.int64)); hq.append(np.full(ln, op in Q_OPS))
            rs.append(np.arange(r, r + ln) if op in R_OPS else np.zeros(ln, np.int64)); hr.append(np.full(ln, op in R_OPS))
        q += ln if op in Q_OPS else 0
        r += ln if op in R_OPS else 0
    return np.concatenate(qs).astype(np.int64), np.concatenate(rs).astype(np.int64), np.concatenate(hq), np.concatenate(hr)


def walk_record(rec, table, seq_pos_off=0, n_like_m=False, ignore_hard_clip=False):
    """rec: dict(pos, flag, cigar [(op, len)], seq bytes of NT16 letters, qual uint8 [len(seq)]) -> dict(snp, allele, qual, seq_pos lists, ref_end).
    The keyword arguments make WRONG models (the tests check that their inputs can tell them from the right one): the read base taken seq_pos_off
    bases further on, N treated as if it were M, the hard-clip shift of a supplementary alignment left out."""
    cigar = [("M" if (n_like_m and op == "N") else op, ln) for op, ln in rec["cigar"]]
    q, r, has_q, has_r = aligned_pairs_full(rec["pos"], cigar)
    both = has_q & has_r
    q, r = q[both], r[both]
    k = np.searchsorted(table.pos, r)
    hit = k < len(table.pos)
    hit[hit] &= table.pos[k[hit]] == r[hit]
    seq = np.frombuffer(rec["seq"], np.uint8)
    hard = 0
    if not ignore_hard_clip and (rec["flag"] & 0x800) and rec["cigar"] and rec["cigar"][0][0] == "H":
        hard = int(rec["cigar"][0][1])
    out = dict(snp=[], allele=[], qual=[], seq_pos=[])
    for qq, kk in zip(q[hit].tolist(), k[hit].tolist()):
        sp = qq + seq_pos_off
        if not 0 <= sp < len(seq):
            continue
        base = seq[sp]
        match = [a for a in range(int(table.n_alleles[kk])) if table.alleles[kk, a] == base]
        if not match:
            continue
        out["snp"].append(kk + 1); out["allele"].append(match[0]); out["qual"].append(int(rec["qual"][sp])); out["seq_pos"].append((sp + hard) & 0xffffffff)
    ref_len = sum(int(ln) for op, ln in rec["cigar"] if op in R_OPS)
    out["ref_end"] = int(rec["pos"]) + (ref_len if ref_len else 1)
    return out


def walk_records(records, tables, **wrong):
    """records: list of dicts with a `contig` index into `tables` -> (cell_off uint64 [n+1], snp uint32, allele uint8, qual uint8, seq_pos uint32, ref_end int64 [n]):
    what floria_hip_pileup_records returns"""
    off, snp, al, qu, sp, re_ = [0], [], [], [], [], []
    for rec in records:
        o = walk_record(rec, tables[rec["contig"]], **wrong)
        snp += o["snp"]; al += o["allele"]; qu += o["qual"]; sp += o["seq_pos"]; re_.append(o["ref_end"])
        off.append(len(snp))
    return (np.asarray(off, np.uint64), np.asarray(snp, np.uint32), np.asarray(al, np.uint8), np.asarray(qu, np.uint8), np.asarray(sp, np.uint32), np.asarray(re_, np.int64))


def changed_records(a, b):
    """indices of the records whose cells or ref_end differ between two results of walk_records"""
    ch = []
    for i in range(len(a[5])):
        la, ha, lb, hb = int(a[0][i]), int(a[0][i + 1]), int(b[0][i]), int(b[0][i + 1])
        same = ha - la == hb - lb and all(np.array_equal(a[f][la:ha], b[f][lb:hb]) for f in (1, 2, 3, 4)) and a[5][i] == b[5][i]
        if not same:
            ch.append(i)
    return ch


# ---- records as bytes ------------------------------------------------------------------------------------------------------------------------
def make_record(pos, cigar, seq, qual=None, flag=0, contig=0, name="r", mapq=60):
    """dict for walk_record plus the BAM record bytes (synth_bam.bam_record: block_size, fixed fields, name, CIGAR words, 4-bit bases, qualities)"""
    seq = NT16[synth_bam._NT16_LUT[np.frombuffer(bytes(seq), np.uint8)]].tobytes() if len(seq) else b""      # what the 4-bit codes of the record decode to (any other letter is N)
    qual = np.full(len(seq), 30, np.uint8) if qual is None else np.asarray(qual, np.uint8)
    assert len(qual) == len(seq)
    raw = synth_bam.bam_record(contig, pos, name, flag, mapq, cigar, seq, qual)
    return dict(pos=int(pos), flag=int(flag), contig=int(contig), cigar=[(op, int(ln)) for op, ln in cigar], seq=seq, qual=qual, name=name, raw=raw)


def pack_records(records, pad=lambda i: 0):
    """BAM record bytes back to back (pad(i) filler bytes in front of record i) -> the keyword arguments of FloriaHip.pileup_records for the records
    (blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off), the offsets read from the records' own fixed fields"""
    blob = bytearray()
    cols = dict(pos=[], flags=[], contig=[], cigar_off=[], n_cigar=[], seq_off=[], l_seq=[], qual_off=[])
    for i, rec in enumerate(records):
        blob += b"\xa5" * pad(i)
        o = len(blob)
        raw = rec["raw"]
        blob += raw
        _bs, _tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", raw, 0)
        c0 = o + 36 + l_name
        s0 = c0 + 4 * n_cig
        cols["pos"].append(pos); cols["flags"].append(flag); cols["contig"].append(rec["contig"]); cols["cigar_off"].append(c0); cols["n_cigar"].append(n_cig)
        cols["seq_off"].append(s0); cols["l_seq"].append(l_seq); cols["qual_off"].append(s0 + (l_seq + 1) // 2)
    dt = dict(pos=np.int32, flags=np.uint16, contig=np.uint32, cigar_off=np.uint64, n_cigar=np.uint32, seq_off=np.uint64, l_seq=np.uint32, qual_off=np.uint64)
    out = {k: np.asarray(v, dt[k]) for k, v in cols.items()}
    out["blob"] = np.frombuffer(bytes(blob), np.uint8)
    return out


def pack_tables(tables):
    """list of SnpTable -> snp_off, snp_pos, alleles, n_alleles of floria_snp_table"""
    off = np.zeros(len(tables) + 1, np.uint64)
    off[1:] = np.cumsum([len(t.pos) for t in tables])
    cat = lambda xs, dt, shape: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
    return dict(snp_off=off, snp_pos=cat([t.pos for t in tables], np.int64, 0), alleles=cat([t.alleles for t in tables], np.uint8, (0, 4)),
                n_alleles=cat([t.n_alleles for t in tables], np.uint8, 0))


def read_vcf_tables(path, contigs):
    """the SNP tables floria makes of a text VCF (file_reader.rs:239-314): records whose alleles are all one letter of ACGT, numbered per contig in file order"""
    rows = {c: [] for c in contigs}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        t = line.rstrip("\n").split("\t")
        al = [t[3]] + ([] if t[4] == "." else t[4].split(","))
        if t[0] in rows and all(len(a) == 1 and a.upper() in "ACGT" for a in al):
            rows[t[0]].append((int(t[1]) - 1, al))
    out = {}
    for c, rs in rows.items():
        out[c] = SnpTable([p for p, _ in rs], [[ord(a) for a in al[:4]] + [0] * (4 - min(4, len(al))) for _, al in rs], [min(len(al), 255) for _, al in rs])
        out[c].all_alleles = [al for _, al in rs]
    return out


# ---- the crafted records (GPU test 1, CPU test b) --------------------------------------------------------------------------------------------
def crafted_case():
    """-> (records, [SnpTable, SnpTable]): every situation the issue lists, two contigs with different tables"""
    rng = np.random.default_rng(20240607)
    # contig 0: SNPs every 10 bases from 100; sites with 1, 3 and 4 alleles, one with a repeated allele byte
    p0 = 100 + 10 * np.arange(400)
    al0 = np.zeros((400, 4), np.uint8); na0 = np.full(400, 2, np.uint8)
    al0[:, 0] = ord("A"); al0[:, 1] = ord("C")
    na0[5] = 1
    al0[6] = [ord("A"), ord("C"), ord("G"), 0]; na0[6] = 3
    al0[7] = [ord("T"), ord("G"), ord("C"), ord("A")]; na0[7] = 4
    al0[8] = [ord("G"), ord("C"), ord("C"), ord("A")]; na0[8] = 4                     # repeated byte: the first match (1) wins
    al0[9] = [ord("a"), ord("c"), 0, 0]                                               # lower case in the table: bytes compare, an upper-case read base matches nothing
    t0 = SnpTable(p0, al0, na0)
    # contig 1: irregular, dense in places
    p1 = np.cumsum(rng.integers(1, 40, size=1500)) + 50
    al1 = np.zeros((1500, 4), np.uint8); al1[:, 0] = ord("G"); al1[:, 1] = ord("T"); al1[::7, 2] = ord("A")
    na1 = np.where(np.arange(1500) % 7 == 0, 3, 2).astype(np.uint8)
    t1 = SnpTable(p1, al1, na1)
    tables = [t0, t1]
    recs = []

    def seq_for(contig, pos, cigar, l_seq=None, other=b"ACGT"):
        """a read whose base at every aligned SNP is drawn from the site's alleles or `other`"""
        q, r, has_q, has_r = aligned_pairs_full(pos, cigar)
        n = sum(ln for op, ln in cigar if op in Q_OPS)
        s = np.frombuffer(other, np.uint8)[rng.integers(0, len(other), size=n)].copy()
        t = tables[contig]
        k = np.searchsorted(t.pos, r)
        ok = has_q & has_r & (k < len(t.pos))
        ok[ok] &= t.pos[k[ok]] == r[ok]
        for qq, kk in zip(q[ok].tolist(), k[ok].tolist()):
            if rng.random() < 0.8:
                s[qq] = t.alleles[kk, rng.integers(0, t.n_alleles[kk])]
        return bytes(s[:n if l_seq is None else l_seq])

    def add(contig, pos, cigar, flag=0, seq=None, qual=None, **kw):
        seq = seq_for(contig, pos, cigar, **kw) if seq is None else seq
        q = rng.integers(0, 60, size=len(seq)).astype(np.uint8) if qual is None else qual
        recs.append(make_record(pos, cigar, seq, q, flag=flag, contig=contig, name="c%d" % len(recs) + "x" * (len(recs) % 4)))
    every = [("S", 3), ("M", 40), ("I", 2), ("M", 30), ("D", 15), ("M", 25), ("N", 60), ("=", 35), ("X", 1), ("P", 2), ("=", 24), ("S", 4), ("H", 6)]
    add(0, 95, every)                                                     # every op; SNPs under D and under N
    add(0, 100, [("M", 11)])                                              # SNP on the first and on the last base of an M run
    add(0, 99, [("M", 1), ("D", 1), ("M", 9), ("N", 1), ("M", 30)])       # SNPs 100 under D, 110 under N
    add(0, 200, [("H", 1200), ("M", 300)], flag=0x800)                    # supplementary with a leading H: shifted seq_pos
    add(0, 200, [("H", 1200), ("M", 300)], flag=0)                        # the same CIGAR without the flag: no shift
    add(0, 200, [("S", 5), ("M", 300), ("H", 7)], flag=0x800)             # the flag without a LEADING H: no shift
    add(0, 130, [("M", 100)], seq=b"T" * 100)                             # T matches no allele of a biallelic A/C site (matches site 7's allele 0)
    add(0, 130, [("M", 100)], seq=b"N" * 100)                             # N bases
    add(0, 130, [("M", 100)], seq=b"=ACMGRSVTWYHKDBN" * 6 + b"ACGT")      # every 4-bit code
    add(0, 140, [("M", 80)], seq=b"")                                     # l_seq = 0
    add(0, 140, [("M", 80)], qual=np.full(80, 255, np.uint8))             # qualities of 0xFF
    add(0, 140, [("M", 80), ("I", 10), ("M", 500)], l_seq=120)            # the CIGAR consumes more query than l_seq
    add(0, 101, [("M", 8)])                                               # no SNP in the span (between 100 and 110)
    add(0, 5000, [("M", 300)])                                            # behind the last SNP altogether
    add(0, 0, [("M", 150)])                                               # starts before the first SNP
    add(0, -1, [("M", 150)])                                              # pos = -1 (an unplaced-style record): reference positions start below 0
    add(0, 4000, [("M", 500)])                                            # ends after the last SNP (4090)
    add(0, 300, [])                                                       # no CIGAR at all: ref_end = pos + 1
    add(0, 300, [("I", 5), ("S", 5)])                                     # consumes no reference
    add(1, 60, [("M", 4000)])                                             # second contig, another table
    add(1, 0, every)
    # chunk borders: n ops of 1M / 1I / 1D patterns with SNPs inside the ops around op 63 / 64 / 65 / 128 / 129
    for n_ops in (63, 64, 65, 129):
        cig = [("M", 7), ("I", 1)] * (n_ops // 2) + ([("M", 9)] if n_ops % 2 else [])
        add(0, 96, cig)                                                   # 7-base runs over a 10-base SNP grid: SNPs fall into the ops at every border
        add(1, 55, [("M", 5), ("D", 2)] * (n_ops // 2) + ([("M", 11)] if n_ops % 2 else []))
    add(0, 90, [("M", 1), ("D", 1), ("M", 1), ("I", 1)] * 1300)           # 5 200 ops
    add(1, 40, [("=", 3), ("X", 1), ("N", 2), ("M", 2), ("S", 0), ("P", 1)] * 900)      # 5 400 ops, zero-length ops among them
    add(0, 50, [("M", 5000)])                                             # one 5000M over 400 SNPs: several trips of 64
    add(1, 45, [("M", 5000)])
    return recs, tables


def random_case(seed=1577, n_records=20000):
    """-> (records, tables): three contigs; short records with dense SNP tables so that every record sees SNPs, every op occurs, and a share of the records
    has more than 64 operations"""
    rng = np.random.default_rng(seed)
    tables = []
    for c, (n_snp, gap) in enumerate(((3000, 6), (1500, 15), (800, 40))):
        pos = np.cumsum(rng.integers(1, 2 * gap, size=n_snp)) + 20
        al = np.frombuffer(b"ACGT", np.uint8)[np.argsort(rng.random((n_snp, 4)), axis=1)].copy()
        na = rng.integers(1, 5, size=n_snp).astype(np.uint8)
        dup = rng.random(n_snp) < 0.05
        al[dup, 2] = al[dup, 1]                                           # repeated allele bytes
        tables.append(SnpTable(pos, al, na))
    letters = np.frombuffer(b"ACGTACGTACGTACGTN=", np.uint8)
    recs = []
    for i in range(n_records):
        c = int(rng.integers(0, 3))
        t = tables[c]
        long_rec = rng.random() < 0.02
        n_ops = int(rng.integers(65, 400)) if long_rec else int(rng.integers(1, 12))
        ops = rng.choice(9, size=n_ops, p=[0.45, 0.08, 0.12, 0.06, 0.04, 0.02, 0.02, 0.14, 0.07])
        lens = rng.integers(1, 8 if long_rec else 40, size=n_ops)
        lens[rng.random(n_ops) < 0.02] = 0
        cigar = [(OPS[o], int(l)) for o, l in zip(ops, lens)]
        pos = int(rng.integers(-5, int(t.pos[-1]) + 30))
        nq = sum(l for o, l in cigar if o in Q_OPS)
        l_seq = nq if rng.random() < 0.9 else int(rng.integers(0, nq + 1))
        seq = bytes(letters[rng.integers(0, len(letters), size=l_seq)])
        qual = rng.integers(0, 256, size=l_seq).astype(np.uint8)
        flag = 0x800 if rng.random() < 0.2 else int(rng.choice([0, 16, 1 | 64, 256]))
        recs.append(make_record(pos, cigar, seq, qual, flag=flag, contig=c, name="r%d" % i))
    return recs, tables


_sweep = []


def random_sweep():
    """random_case() and its walk -> (records, tables, walked): computed once per process and shared by the tests, never changed"""
    if not _sweep:
        recs, tables = random_case()
        _sweep.append((recs, tables, walk_records(recs, tables)))
    return _sweep[0]


def coverage(records, tables, result):
    """what the random sweep asserts about its own input: ops seen, cells, SNPs under D / N, records with more than 64 ops"""
    ops = set(op for r in records for op, _ in r["cigar"])
    under = 0
    for r in records:
        t = tables[r["contig"]]
        ref = r["pos"]
        for op, ln in r["cigar"]:
            if op in ("D", "N"):
                under += int(np.searchsorted(t.pos, ref + ln) - np.searchsorted(t.pos, ref))
            ref += ln if op in R_OPS else 0
    return dict(ops=ops, cells=int(result[0][-1]), under_dn=under, long_records=sum(1 for r in records if len(r["cigar"]) > 64))
