"""A/B at ABI level: (A) pileup_records_realign + host marshal + upload_batch_packed against (B) pileup_records_resident + assemble_contigs on the
long-read set of scripts/cli_timing.py (config 4, scale 0.5).  usage: python scripts/assemble_ab.py N_CONTIGS N_RUNS   (profiles/assemble_resident.md: 200 5)"""
import os
import sys
import time
import multiprocessing as mp

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floria_amd import synth, synth_bam  # noqa: E402


def make_contig(i):
    c = synth.make_config_contig(4, i, 0.5, keep_layout=True)
    d = synth_bam.contig_dataset(c, np.random.default_rng(1000 + i), sub_rate=0.0)
    raws, pos, l_name, n_cig, l_seq = [], [], [], [], []
    for name, cells, span, recs_r, _ in d["reads"]:
        for p, raw, seq, cigar in recs_r:
            raws.append(raw); pos.append(p); l_name.append(len(name) + 1); n_cig.append(len(cigar)); l_seq.append(len(seq))
    return (b"".join(raws), np.asarray([len(r) for r in raws], np.int64), np.asarray(pos, np.int32), np.asarray(l_name, np.int64), np.asarray(n_cig, np.uint32),
            np.asarray(l_seq, np.uint32), d["ref"], d["snps"])


def main():
    n_contigs, n_runs = int(sys.argv[1]), int(sys.argv[2])
    t0 = time.time()
    with mp.Pool(16) as pool:                              # (before anything initialises HIP in this process)
        parts = pool.map(make_contig, range(n_contigs), chunksize=1)
    print(f"data set: {n_contigs} contigs generated in {time.time() - t0:.1f}s", flush=True)
    blob = np.frombuffer(b"".join(p[0] for p in parts), np.uint8)
    sizes = np.concatenate([p[1] for p in parts])
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    pos = np.concatenate([p[2] for p in parts]); l_name = np.concatenate([p[3] for p in parts]); n_cig = np.concatenate([p[4] for p in parts]); l_seq = np.concatenate([p[5] for p in parts])
    contig = np.repeat(np.arange(n_contigs, dtype=np.uint32), [len(p[2]) for p in parts])
    cigar_off = (start + 36 + l_name).astype(np.uint64); seq_off = cigar_off + 4 * n_cig.astype(np.uint64); qual_off = seq_off + (l_seq.astype(np.uint64) + 1) // 2
    flags = np.zeros(len(pos), np.uint16)
    snp_off = np.zeros(n_contigs + 1, np.uint64); snp_off[1:] = np.cumsum([len(p[7]) for p in parts])
    snp_pos = np.asarray([s[0] for p in parts for s in p[7]], np.int64)
    alleles = np.zeros((len(snp_pos), 4), np.uint8)
    alleles[:, 0] = [ord(s[1]) for p in parts for s in p[7]]; alleles[:, 1] = [ord(s[2]) for p in parts for s in p[7]]
    n_alleles = np.full(len(snp_pos), 2, np.uint8)
    ref_off = np.zeros(n_contigs + 1, np.uint64); ref_off[1:] = np.cumsum([len(p[6]) for p in parts])
    ref_seq = np.frombuffer(b"".join(p[6] for p in parts), np.uint8)
    del parts
    n = len(pos)
    kw = dict(blob=blob, pos=pos, flags=flags, contig=contig, cigar_off=cigar_off, n_cigar=n_cig, seq_off=seq_off, l_seq=l_seq, qual_off=qual_off,
              snp_off=snp_off, snp_pos=snp_pos, alleles=alleles, n_alleles=n_alleles, ref_off=ref_off, ref_seq=ref_seq)
    in_bytes = sum(v.nbytes for v in kw.values())
    print(f"{n} records, blob {blob.nbytes >> 20} MiB, {len(snp_pos)} SNPs, reference {ref_seq.nbytes >> 10} KiB, inputs {in_bytes} B", flush=True)

    from floria_amd import lib
    from floria_amd.pileup import Pileup
    ctx = lib.FloriaHip(0)
    tm = lambda: {k: round(v, 3) if isinstance(v, float) else v for k, v in ctx.timing().items() if k in ("h2d_ms", "d2h_ms", "pileup_ms", "select_ms", "total_ms", "upload_pinned_bytes", "upload_staged_bytes")}

    def order_of(first, last, has):
        """records with cells, by (contig, first ascending, last descending, index): every long read is a one-part fragment"""
        idx = np.nonzero(has)[0]
        o = np.lexsort((idx, -last[idx].astype(np.int64), first[idx].astype(np.int64), contig[idx]))
        return idx[o]

    def route_a():
        w = {}
        t = time.perf_counter()
        (cell_off, snp, allele, qual, seq_pos, ref_end), counts = ctx.pileup_records_realign(**kw)
        w["pileup_call"] = time.perf_counter() - t; w["pileup_timing"] = tm()
        t = time.perf_counter()
        lens = np.diff(cell_off).astype(np.int64)
        has = lens > 0
        co = cell_off.astype(np.int64)
        first = np.where(has, snp[np.minimum(co[:-1], len(snp) - 1)], 0); last = np.where(has, snp[np.maximum(co[1:], 1) - 1], 0)
        order = order_of(first, last, has)
        ln = lens[order]
        new_off = np.concatenate([[0], np.cumsum(ln)])
        src = np.repeat(co[:-1][order] - new_off[:-1], ln) + np.arange(new_off[-1])
        s2, a2, q2 = snp[src], allele[src], qual[src]
        rc = np.searchsorted(contig[order], np.arange(n_contigs + 1))          # reads per contig
        pileups = []
        for c in range(n_contigs):
            r0, r1 = rc[c], rc[c + 1]
            c0, c1 = new_off[r0], new_off[r1]
            pileups.append(Pileup((new_off[r0:r1 + 1] - c0).astype(np.uint32), s2[c0:c1], a2[c0:c1], q2[c0:c1], first[order[r0:r1]].astype(np.uint32), last[order[r0:r1]].astype(np.uint32)))
        w["marshal"] = time.perf_counter() - t
        t = time.perf_counter()
        arena, parr, packed_bytes = lib.pack_pileups(pileups, pinned=True)
        w["pack"] = time.perf_counter() - t
        t = time.perf_counter()
        batch = ctx.upload_batch_packed(parr)
        w["upload_call"] = time.perf_counter() - t; w["upload_timing"] = tm()
        w["cells"] = int(cell_off[-1]); w["merged_cells"] = int(new_off[-1]); w["reads"] = len(order)
        w["d2h_bytes"] = 10 * int(cell_off[-1]) + 8 * (n + 1) + 8 * n + 40; w["h2d_bytes"] = in_bytes + packed_bytes
        w["total"] = w["pileup_call"] + w["marshal"] + w["pack"] + w["upload_call"]
        return w, batch, arena, pileups

    def route_b():
        w = {}
        t = time.perf_counter()
        s = ctx.pileup_records_resident(**kw)
        w["pileup_call"] = time.perf_counter() - t; w["pileup_timing"] = tm()
        t = time.perf_counter()
        has = s.cell_off[1:] > s.cell_off[:-1]
        order = order_of(s.first_snp, s.last_snp, has)
        frag_off = np.searchsorted(contig[order], np.arange(n_contigs + 1)).astype(np.uint64)
        part_off = np.arange(len(order) + 1, dtype=np.uint64)
        w["plan"] = time.perf_counter() - t
        t = time.perf_counter()
        got = ctx.assemble_contigs(s, frag_off, part_off, order.astype(np.uint32))
        w["assemble_call"] = time.perf_counter() - t; w["assemble_timing"] = tm()
        w["reads"] = len(order)
        w["d2h_bytes"] = 8 * (n + 1) + 8 * n + 8 * n + 40 + 8 * (n_contigs + 1) + 24 * n_contigs
        w["h2d_bytes"] = in_bytes + 8 * (len(order) + 1) + 8 * len(order) + 8 * (n_contigs + 1) + (80 + 8 + 24) * n_contigs
        w["total"] = w["pileup_call"] + w["plan"] + w["assemble_call"]
        s.free()
        return w, got

    res = {"A": [], "B": []}
    for run in range(n_runs + 1):                          # run 0 warms up both routes (allocations) and checks that they agree
        wa, batch, arena, pileups = route_a()
        wb, got = route_b()
        if run == 0:
            h = (lib.C.c_void_p * n_contigs)(*[batch._arr[i] for i in range(n_contigs)])
            for c in (0, n_contigs // 2, n_contigs - 1):
                p = pileups[c]
                ua = lib.ResidentContig(ctx, handle=lib.C.c_void_p(h[c]), n_reads=p.n_reads)
                for f, cnt in (("read_off", p.n_reads + 1), ("first", p.n_reads), ("last", p.n_reads), ("snp", p.n_cells), ("cell_aw", p.n_cells), ("tw", 2 * p.n_reads), ("meta", 8 * p.n_reads)):
                    assert np.array_equal(ua.download(f, cnt), got[c].download(f, cnt)), (c, f)
                ua._h = None
            print("routes agree on contigs 0, middle, last (all seven fields)", flush=True)
        else:
            res["A"].append(wa); res["B"].append(wb)
        print(f"run {run}: A {wa['total'] * 1e3:.1f} ms  B {wb['total'] * 1e3:.1f} ms", flush=True)
        print("  A", wa, flush=True); print("  B", wb, flush=True)
        batch.free(); arena.free()
        for g in got:
            g.free()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for r in ("A", "B"):
        keys = [k for k, v in res[r][0].items() if isinstance(v, float)]
        print(r, "median of", n_runs, ":", {k: round(med([w[k] for w in res[r]]) * 1e3, 2) for k in keys}, "ms; bytes h2d", res[r][0]["h2d_bytes"], "d2h", res[r][0]["d2h_bytes"], flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
