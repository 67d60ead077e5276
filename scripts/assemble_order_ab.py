"""A/B at ABI level on paired short reads (config 3, scale 0.5: every fragment has two parts): after one pileup_records_resident,
  (P) assemble_contigs, no set order — the call as it was before floria_hip_assemble_contigs_ordered existed: the baseline (its S1 in "arith" = 1 would emulate
      one-walk sets, which is not what the reference computes for these fragments);
  (H) assemble_contigs with a host-given set_order.  The order is computed OUTSIDE the timed region (from a downloaded copy of the cells, with the CPU oracle):
      the replay a real host would have to do, and the download it needs, are NOT in this route's figure;
  (D) assemble_contigs_ordered: the order derived on the device.
usage: python scripts/assemble_order_ab.py N_CONTIGS N_RUNS   (profiles/assemble_set_order.md: 60 5)"""
import os
import sys
import time
import multiprocessing as mp

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floria_amd import synth, synth_bam  # noqa: E402

FAST_CELLS = 223          # csrc/assemble_order_kernel.h: AO_FAST_CELLS


def make_contig(i):
    c = synth.make_config_contig(3, i, 0.5, keep_layout=True)
    d = synth_bam.contig_dataset(c, np.random.default_rng(3000 + i), sub_rate=0.0)
    raws, pos, l_name, n_cig, l_seq, flags, read = [], [], [], [], [], [], []
    for r, (name, cells, span, recs_r, _) in enumerate(d["reads"]):
        for k, (p, raw, seq, cigar) in enumerate(recs_r):
            raws.append(raw); pos.append(p); l_name.append(len(name) + 1); n_cig.append(len(cigar)); l_seq.append(len(seq)); read.append(r)
            flags.append(1 | 2 | (64 | 32 if k == 0 else 128 | 16))
    return (b"".join(raws), np.asarray([len(r) for r in raws], np.int64), np.asarray(pos, np.int32), np.asarray(l_name, np.int64), np.asarray(n_cig, np.uint32),
            np.asarray(l_seq, np.uint32), d["ref"], d["snps"], np.asarray(flags, np.uint16), np.asarray(read, np.int64))


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
    flags = np.concatenate([p[8] for p in parts])
    read_base = np.concatenate([[0], np.cumsum([int(p[9].max()) + 1 for p in parts])])
    read_of = np.concatenate([p[9] + read_base[i] for i, p in enumerate(parts)])          # the read (pair) of every record; its records are consecutive, mate 1 first
    snp_off = np.zeros(n_contigs + 1, np.uint64); snp_off[1:] = np.cumsum([len(p[7]) for p in parts])
    snp_pos = np.asarray([s[0] for p in parts for s in p[7]], np.int64)
    alleles = np.zeros((len(snp_pos), 4), np.uint8)
    alleles[:, 0] = [ord(s[1]) for p in parts for s in p[7]]; alleles[:, 1] = [ord(s[2]) for p in parts for s in p[7]]
    n_alleles = np.full(len(snp_pos), 2, np.uint8)
    del parts
    n = len(pos)
    kw = dict(blob=blob, pos=pos, flags=flags, contig=contig, cigar_off=cigar_off, n_cigar=n_cig, seq_off=seq_off, l_seq=l_seq, qual_off=qual_off,
              snp_off=snp_off, snp_pos=snp_pos, alleles=alleles, n_alleles=n_alleles)
    print(f"{n} records of {int(read_of[-1]) + 1} pairs, blob {blob.nbytes >> 20} MiB, {len(snp_pos)} SNPs", flush=True)

    from floria_amd import lib
    from oracle import oracle
    oracle.build()
    ctx = lib.FloriaHip(0)
    tm = lambda: {k: round(v, 3) if isinstance(v, float) else v for k, v in ctx.timing().items() if k in ("h2d_ms", "d2h_ms", "pileup_ms", "select_ms", "total_ms", "upload_pinned_bytes", "upload_staged_bytes")}

    # ---- outside every timed region: the plan, and the host-given order from a downloaded copy of the cells ----
    cell_off, snp = ctx.pileup_records(**kw)[:2]
    co = cell_off.astype(np.int64)
    lens = np.diff(co)
    n_reads_all = int(read_of[-1]) + 1
    rec0 = np.searchsorted(read_of, np.arange(n_reads_all + 1))                           # records of read r: [rec0[r], rec0[r + 1])
    cells_of_read = np.add.reduceat(lens, rec0[:-1])
    keep = np.nonzero(cells_of_read > 0)[0]
    has = lens > 0
    big = np.iinfo(np.int64).max
    first_rec = np.where(has, snp[np.minimum(co[:-1], len(snp) - 1)].astype(np.int64), big); last_rec = np.where(has, snp[np.maximum(co[1:], 1) - 1].astype(np.int64), -1)
    first = np.minimum.reduceat(first_rec, rec0[:-1])[keep]; last = np.maximum.reduceat(last_rec, rec0[:-1])[keep]
    ctg = contig[rec0[:-1]][keep]
    o = np.lexsort((keep, -last, first, ctg))
    frags = keep[o]                                                                          # reads in Frag::cmp order, contig by contig
    frag_off = np.searchsorted(ctg[o], np.arange(n_contigs + 1)).astype(np.uint64)
    n_parts = (rec0[1:] - rec0[:-1])[frags]
    part_off = np.concatenate([[0], np.cumsum(n_parts)]).astype(np.uint64)
    part_rec = (np.repeat(rec0[:-1][frags] - part_off[:-1].astype(np.int64), n_parts) + np.arange(int(part_off[-1]))).astype(np.uint32)
    t0 = time.time()
    so, n_differ, n_general, n_two = [], 0, 0, 0
    for f, r in enumerate(frags):
        segs = [snp[co[i]:co[i + 1]] for i in range(rec0[r], rec0[r + 1]) if lens[i]]
        merged = np.unique(np.concatenate(segs))
        so.append(oracle.set_order_of(merged, segs))
        n_differ += not np.array_equal(so[-1], oracle.set_order_of(merged, [merged]))
        n_general += sum(len(s) for s in segs) > FAST_CELLS
        n_two += len(segs) >= 2
    set_order = np.concatenate(so).astype(np.uint32)
    print(f"{len(frags)} fragments, {n_two} with two parts that have cells, {len(set_order)} merged cells; host replay of the set orders (CPU oracle, not timed below): {time.time() - t0:.1f}s", flush=True)
    print(f"fragment orders that differ from the one-walk order: {n_differ} of {len(frags)}; fragments beyond the wavefront kernel (general path): {n_general} of {len(frags)}", flush=True)
    plan_bytes = frag_off.nbytes + part_off.nbytes + part_rec.nbytes + 4 * len(frags)      # (+ the fragments' contigs, which the library derives and sends)
    cell_counts = np.diff(np.concatenate([[0], np.cumsum([len(x) for x in so])])[frag_off.astype(np.int64)])

    def route(kind, s):
        w = {}
        t = time.perf_counter()
        if kind == "D":
            got = ctx.assemble_contigs_ordered(s, frag_off, part_off, part_rec)
        else:
            got = ctx.assemble_contigs(s, frag_off, part_off, part_rec, set_order=set_order if kind == "H" else None)
        w["call"] = time.perf_counter() - t
        w["timing"] = tm()
        w["h2d_bytes"] = plan_bytes + (set_order.nbytes if kind == "H" else 0) + (4 * n_contigs if kind == "D" else 0)
        w["d2h_bytes"] = 8 * (n_contigs + 1) + 40 * n_contigs + (8 if kind != "P" else 0)   # cell totals, flatten status, (the permutation check's word)
        return w, got

    res = {"P": [], "H": [], "D": []}
    s = ctx.pileup_records_resident(**kw)
    for run in range(n_runs + 1):                          # run 0 warms up (allocations) and checks the derived orders against the host's
        for kind in (("P", "H", "D"), ("H", "D", "P"), ("D", "P", "H"))[run % 3]:
            w, got = route(kind, s)
            if run == 0 and kind == "D":
                for c in range(n_contigs):
                    a = int(np.concatenate([[0], np.cumsum(cell_counts)])[c])
                    assert np.array_equal(got[c].download("set_order", int(cell_counts[c])), set_order[a:a + int(cell_counts[c])]), c
                print("the derived set orders of all contigs equal the host's", flush=True)
            if run:
                res[kind].append(w)
            print(f"run {run} {kind}: {w['call'] * 1e3:.2f} ms", w, flush=True)
            for g in got:
                g.free()
    s.free()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for kind in ("P", "H", "D"):
        keys = ("h2d_ms", "d2h_ms", "pileup_ms", "select_ms", "total_ms")
        print(kind, "median of", n_runs, ": call", round(med([w["call"] for w in res[kind]]) * 1e3, 3), "ms;", {k: round(med([w["timing"][k] for w in res[kind]]), 3) for k in keys},
              "; bytes h2d", res[kind][0]["h2d_bytes"], "d2h", res[kind][0]["d2h_bytes"], flush=True)
    d = med([w["timing"]["pileup_ms"] for w in res["D"]]) - med([w["timing"]["pileup_ms"] for w in res["P"]])
    print(f"the new launches (preset + assemble_order_kernel + general kernel): pileup_ms(D) - pileup_ms(P) = {d:.3f} ms", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
