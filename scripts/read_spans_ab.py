"""Read positions on resident contigs, at ABI level, on the long-read set of scripts/assemble_ab.py (config 4, scale 0.5; every long read a one-part fragment):
  (a) floria_hip_assemble_contigs (plain) of this tree against the same call of another tree (the parent commit, built beside it), alternating, one process each;
  (b) the cost of FLORIA_ASM_KEEP_SEQ_POS over the plain call, and the arena bytes with and without;
  (c) floria_hip_read_spans, one query per read with its range = the read's own span, against what a host does today: floria_hip_pileup_records and its download;
  (d) floria_hip_drop_monomorphic on contigs with and without positions.
usage: python scripts/read_spans_ab.py N_CONTIGS N_RUNS [PARENT_TREE]      (profiles/read_spans.md: 200 5 scripts/tmp_prev/parent)
PARENT_TREE holds floria_amd/ of the other commit with its library built (git archive HEAD floria_amd include | tar -x -C DIR; make -C DIR/floria_amd/csrc); without it (a) is left out."""
import json
import os
import subprocess
import sys
import time
import multiprocessing as mp

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_contig(i):
    from floria_amd import synth, synth_bam
    c = synth.make_config_contig(4, i, 0.5, keep_layout=True)
    d = synth_bam.contig_dataset(c, np.random.default_rng(1000 + i), sub_rate=0.0)
    raws, pos, l_name, n_cig, l_seq = [], [], [], [], []
    for name, cells, span, recs_r, _ in d["reads"]:
        for p, raw, seq, cigar in recs_r:
            raws.append(raw); pos.append(p); l_name.append(len(name) + 1); n_cig.append(len(cigar)); l_seq.append(len(seq))
    return (b"".join(raws), np.asarray([len(r) for r in raws], np.int64), np.asarray(pos, np.int32), np.asarray(l_name, np.int64), np.asarray(n_cig, np.uint32),
            np.asarray(l_seq, np.uint32), len(d["ref"]), d["snps"])


def data_set(n_contigs):
    with mp.Pool(16) as pool:                              # (before anything initialises HIP in this process)
        parts = pool.map(make_contig, range(n_contigs), chunksize=1)
    blob = np.frombuffer(b"".join(p[0] for p in parts), np.uint8)
    sizes = np.concatenate([p[1] for p in parts])
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    pos = np.concatenate([p[2] for p in parts]); l_name = np.concatenate([p[3] for p in parts]); n_cig = np.concatenate([p[4] for p in parts]); l_seq = np.concatenate([p[5] for p in parts])
    contig = np.repeat(np.arange(n_contigs, dtype=np.uint32), [len(p[2]) for p in parts])
    cigar_off = (start + 36 + l_name).astype(np.uint64); seq_off = cigar_off + 4 * n_cig.astype(np.uint64); qual_off = seq_off + (l_seq.astype(np.uint64) + 1) // 2
    snp_off = np.zeros(n_contigs + 1, np.uint64); snp_off[1:] = np.cumsum([len(p[7]) for p in parts])
    snp_pos = np.asarray([s[0] for p in parts for s in p[7]], np.int64)
    alleles = np.zeros((len(snp_pos), 4), np.uint8)
    alleles[:, 0] = [ord(s[1]) for p in parts for s in p[7]]; alleles[:, 1] = [ord(s[2]) for p in parts for s in p[7]]
    return dict(blob=blob, pos=pos, flags=np.zeros(len(pos), np.uint16), contig=contig, cigar_off=cigar_off, n_cigar=n_cig, seq_off=seq_off, l_seq=l_seq, qual_off=qual_off,
                snp_off=snp_off, snp_pos=snp_pos, alleles=alleles, n_alleles=np.full(len(snp_pos), 2, np.uint8))


def plan_of(s, contig, n_contigs):
    """records with cells, by (contig, first ascending, last descending, index): every long read is a one-part fragment"""
    has = s.cell_off[1:] > s.cell_off[:-1]
    idx = np.nonzero(has)[0]
    o = np.lexsort((idx, -s.last_snp[idx].astype(np.int64), s.first_snp[idx].astype(np.int64), contig[idx]))
    order = idx[o]
    return order, np.searchsorted(contig[order], np.arange(n_contigs + 1)).astype(np.uint64), np.arange(len(order) + 1, dtype=np.uint64)


def arena_bytes(R, C, n, sp):
    seg = lambda b: (b + 255) & ~255
    return seg(4 * (R + n)) + 2 * seg(4 * R) + 2 * seg(4 * C + 16) + seg(16 * R) + seg(32 * R) + (seg(4 * C + 16) if sp else 0)


med = lambda xs: sorted(xs)[len(xs) // 2]


def timed(ctx, f):
    t = time.perf_counter()
    r = f()
    w = (time.perf_counter() - t) * 1e3
    tm = ctx.timing()
    return r, dict(call_ms=w, **{k: tm[k] for k in ("h2d_ms", "d2h_ms", "pileup_ms", "select_ms", "total_ms")})


def child_plain(n_contigs):
    """one process of (a): a residency, one warm-up, then three plain assemble calls; prints the median call as one JSON line"""
    kw = data_set(n_contigs)
    from floria_amd import lib
    ctx = lib.FloriaHip(0)
    s = ctx.pileup_records_resident(**kw)
    order, frag_off, part_off = plan_of(s, kw["contig"], n_contigs)
    runs = []
    for k in range(4):
        got, w = timed(ctx, lambda: ctx.assemble_contigs(s, frag_off, part_off, order.astype(np.uint32)))
        for g in got:
            g.free()
        if k:
            runs.append(w)
    print("RESULT " + json.dumps({k: med([r[k] for r in runs]) for k in runs[0]}), flush=True)
    s.free(); ctx.close()


def child_full(n_contigs, n_runs):
    kw = data_set(n_contigs)
    n = len(kw["pos"])
    print(f"{n} records, blob {kw['blob'].nbytes >> 20} MiB, {len(kw['snp_pos'])} SNPs", flush=True)
    from floria_amd import lib
    ctx = lib.FloriaHip(0)
    counts = np.diff(kw["snp_off"]).astype(np.uint64)
    res = {k: [] for k in ("asm_plain", "asm_keep", "mono_plain", "mono_keep", "spans", "host_pileup_records")}
    for run in range(n_runs + 1):                          # run 0 warms up (allocations) and checks the answers
        s = ctx.pileup_records_resident(**kw)
        order, frag_off, part_off = plan_of(s, kw["contig"], n_contigs)
        pr = order.astype(np.uint32)
        R, C = len(order), int((s.cell_off[1:] - s.cell_off[:-1])[order].sum())
        first_two = [("asm_plain", False), ("asm_keep", True)]
        handles = {}
        for name, keep in (first_two if run % 2 == 0 else first_two[::-1]):          # the routes alternate
            handles[name], w = timed(ctx, lambda: ctx.assemble_contigs(s, frag_off, part_off, pr, keep_seq_pos=keep))
            res[name].append(w)
        for name, src in (("mono_plain", "asm_plain"), ("mono_keep", "asm_keep")) if run % 2 == 0 else (("mono_keep", "asm_keep"), ("mono_plain", "asm_plain")):
            (batch, r), w = timed(ctx, lambda: ctx.drop_monomorphic(handles[src], counts, 0.03125))
            w["device_ms_by_kind"] = ctx.mono_timing(); w["out_cells"] = C - r["n_removed_cells"]
            res[name].append(w)
            batch.free()
        # one query per read, its range = the read's own span: one group per read
        gc = kw["contig"][order].astype(np.uint32)
        rd = (np.arange(R) - frag_off[gc].astype(np.int64)).astype(np.uint32)
        ranges = np.stack([s.first_snp[order], s.last_snp[order]], axis=1)
        groups = (np.arange(R + 1, dtype=np.uint64), rd)
        t = time.perf_counter()
        left, right = ctx.read_spans(handles["asm_keep"], gc, groups, ranges)
        w = dict(call_ms=(time.perf_counter() - t) * 1e3, **{k: v for k, v in ctx.timing().items() if k in ("h2d_ms", "d2h_ms", "pileup_ms", "total_ms")})
        w["d2h_bytes"] = 8 * R; w["h2d_bytes"] = 4 * R + 8 * (R + 1) + 4 * R + 8 * R + 40 * n_contigs
        res["spans"].append(w)
        for hs in handles.values():
            for h in hs:
                h.free()
        s.free()
        # what a host does today: the cells come down (floria_hip_pileup_records returns snp, allele, qual, seq_pos, 10 B per cell; snp + seq_pos are 8 of them)
        t = time.perf_counter()
        cell_off, snp, allele, qual, seq_pos, ref_end = ctx.pileup_records(**kw)
        w = dict(call_ms=(time.perf_counter() - t) * 1e3, **{k: v for k, v in ctx.timing().items() if k in ("h2d_ms", "d2h_ms", "pileup_ms", "total_ms")})
        w["d2h_bytes_snp_seq_pos"] = 8 * int(cell_off[-1]); w["d2h_bytes"] = 10 * int(cell_off[-1]) + 8 * (n + 1) + 8 * n
        res["host_pileup_records"].append(w)
        if run == 0:
            co = cell_off.astype(np.int64)
            assert np.array_equal(left, seq_pos[co[:-1][order]]) and np.array_equal(right, seq_pos[co[1:][order] - 1]), "read_spans against the downloaded map"
            print(f"read_spans agrees with the downloaded seq_pos for all {R} reads; {C} cells; arena bytes {arena_bytes(R, C, n_contigs, False)} plain, {arena_bytes(R, C, n_contigs, True)} with positions", flush=True)
        print(f"run {run}: " + "  ".join(f"{k} {v[-1]['call_ms']:.2f}" for k, v in res.items()), flush=True)
    for k, v in res.items():
        v = v[1:]
        print(k, "median of", n_runs, ":", {f: round(med([x[f] for x in v]), 3) for f in v[0] if isinstance(v[0][f], float)},
              {f: v[0][f] for f in v[0] if isinstance(v[0][f], int)}, flush=True)
    last = res["mono_keep"][-1]["device_ms_by_kind"], res["mono_plain"][-1]["device_ms_by_kind"]
    print("drop_monomorphic device ms by kind, last run: with positions", {k: round(x, 3) for k, x in last[0].items()}, "without", {k: round(x, 3) for k, x in last[1].items()}, flush=True)
    ctx.close()


def main():
    if sys.argv[1] == "--child":
        sys.path.insert(0, sys.argv[3])
        return child_plain(int(sys.argv[4])) if sys.argv[2] == "plain" else child_full(int(sys.argv[4]), int(sys.argv[5]))
    n_contigs, n_runs = int(sys.argv[1]), int(sys.argv[2])
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None

    def child(*args):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *[str(a) for a in args]], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit(f"child {args} failed with status {out.returncode}:\n{out.stdout}\n{out.stderr}")          # (nothing more is started)
        return out.stdout

    if parent:
        rows = {"parent": [], "this": []}
        for run in range(n_runs):
            for name, root in (("parent", parent), ("this", ROOT)) if run % 2 == 0 else (("this", ROOT), ("parent", parent)):
                line = [l for l in child("plain", root, n_contigs).splitlines() if l.startswith("RESULT ")][0]
                rows[name].append(json.loads(line[7:]))
                print(f"(a) run {run} {name}: {rows[name][-1]}", flush=True)
        for name in rows:
            calls = [r["call_ms"] for r in rows[name]]
            print(f"(a) {name}: call_ms median {med(calls):.3f}, min {min(calls):.3f}, max {max(calls):.3f}, spread {max(calls) - min(calls):.3f}; "
                  f"total_ms median {med([r['total_ms'] for r in rows[name]]):.3f}, pileup_ms median {med([r['pileup_ms'] for r in rows[name]]):.3f}", flush=True)
    print(child("full", ROOT, n_contigs, n_runs), flush=True)


if __name__ == "__main__":
    main()
