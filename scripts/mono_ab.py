"""A/B at ABI level for --ignore-monomorphic on RESIDENT contigs: (A) the host route — download the cells, filter them in numpy (remove_monomorphic_allele,
utils_frags.rs:713-772, vectorised), pack, packed upload — against (B) floria_hip_drop_monomorphic on the handles, on the pileups of the long-read set of
scripts/assemble_ab.py (config 4, scale 0.5) at epsilon 0.03125.  The two routes alternate; medians over the runs behind a warm-up run that also checks that
they agree.  usage: python scripts/mono_ab.py N_CONTIGS N_RUNS   (profiles/drop_monomorphic.md: 200 5)"""
import os
import sys
import time
import multiprocessing as mp

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floria_amd import synth  # noqa: E402

EPS = 0.03125


def make_contig(i):
    c = synth.make_config_contig(4, i, 0.5)
    return c.pileup, len(c.snp_pos)


def weight_table(src, pileups):
    """Q24 weight of every quality byte the data set uses, read off the resident cells (what the library's flatten made of them); -1 for unused bytes"""
    w = np.full(256, -1, np.int64)
    for c, p in zip(src, pileups):
        w[p.qual] = (c.download("cell_aw", p.n_cells) & 0x0fffffff).astype(np.int64)
    return w


def host_filter(off, snp, aw, n, w_sorted, q_of):
    """remove_monomorphic_allele over one contig's downloaded resident arrays -> the filtered Pileup"""
    from floria_amd.pileup import Pileup
    al, wt = (aw >> 28).astype(np.int64), (aw & 0x0fffffff).astype(np.int64)
    s = snp.astype(np.int64) - 1
    sums = np.bincount(4 * s + al, weights=wt.astype(np.float64), minlength=4 * n).reshape(n, 4)      # (exact: integers below 2^53)
    key = np.bincount(4 * s + al, minlength=4 * n).reshape(n, 4) > 0
    top = np.sort(np.where(key, sums, -1.0), axis=1)[:, ::-1]
    nkey = key.sum(axis=1)
    gone = (nkey == 1) | ((nkey >= 2) & ((top[:, 0] * 2.0 ** -24) * EPS > top[:, 1] * 2.0 ** -24))
    keep = ~gone[s]
    read = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    kept = np.bincount(read[keep], minlength=len(off) - 1)
    alive = np.nonzero(kept)[0]
    new_off = np.concatenate([[0], np.cumsum(kept[alive])])
    ks, ka, kq = snp[keep], al[keep].astype(np.uint8), q_of[np.searchsorted(w_sorted, wt[keep])].astype(np.uint8)
    first, last = ks[new_off[:-1]], ks[new_off[1:] - 1]
    order = np.lexsort((alive, -last.astype(np.int64), first.astype(np.int64)))
    ln = kept[alive][order]
    off2 = np.concatenate([[0], np.cumsum(ln)])
    take = np.repeat(new_off[:-1][order] - off2[:-1], ln) + np.arange(off2[-1])
    return Pileup(off2.astype(np.uint32), ks[take], ka[take], kq[take], first[order], last[order])


def main():
    n_contigs, n_runs = int(sys.argv[1]), int(sys.argv[2])
    t0 = time.time()
    with mp.Pool(16) as pool:                              # (before anything initialises HIP in this process)
        parts = pool.map(make_contig, range(n_contigs), chunksize=1)
    pileups, counts = [p[0] for p in parts], [p[1] for p in parts]
    R, CELLS, S = sum(p.n_reads for p in pileups), sum(p.n_cells for p in pileups), sum(counts)
    print(f"data set: {n_contigs} contigs, {R} reads, {CELLS} cells, {S} SNPs, generated in {time.time() - t0:.1f}s", flush=True)

    from floria_amd import lib
    ctx = lib.FloriaHip(0)
    src = ctx.upload_batch(pileups)
    w24 = weight_table(src, pileups)
    w_sorted, q_of = np.unique(w24, return_index=True)       # weight -> a quality byte with that weight
    keys = ("h2d_ms", "d2h_ms", "pileup_ms", "select_ms", "total_ms", "upload_pinned_bytes", "upload_staged_bytes")
    tm = lambda: {k: round(v, 3) if isinstance(v, float) else v for k, v in ctx.timing().items() if k in keys}

    def route_a():
        w = {}
        t = time.perf_counter()
        cells = [(c.download("read_off", p.n_reads + 1), c.download("snp", p.n_cells), c.download("cell_aw", p.n_cells)) for c, p in zip(src, pileups)]
        w["download"] = time.perf_counter() - t
        t = time.perf_counter()
        out = [host_filter(off, snp, aw, n, w_sorted, q_of) for (off, snp, aw), n in zip(cells, counts)]
        w["filter"] = time.perf_counter() - t
        t = time.perf_counter()
        arena, parr, packed_bytes = lib.pack_pileups(out, pinned=True)
        w["pack"] = time.perf_counter() - t
        t = time.perf_counter()
        batch = ctx.upload_batch_packed(parr)
        w["upload_call"] = time.perf_counter() - t; w["upload_timing"] = tm()
        w["d2h_bytes"] = 8 * CELLS + 4 * (R + n_contigs); w["h2d_bytes"] = packed_bytes
        w["total"] = w["download"] + w["filter"] + w["pack"] + w["upload_call"]
        return w, batch, arena, out

    def route_b():
        w = {}
        t = time.perf_counter()
        batch, res = ctx.drop_monomorphic(src, counts, EPS)
        w["drop_call"] = time.perf_counter() - t; w["drop_timing"] = dict(tm(), **ctx.mono_timing())
        r_out = int(res["read_off"][-1])
        w["d2h_bytes"] = 12 * R + 8 * n_contigs + 24 * n_contigs + S          # three words per read, the removed counts, the status words, the mask of the result
        w["h2d_bytes"] = 4 * (r_out + n_contigs) + 4 * r_out + (48 + 16 + 8 + 80 + 8 + 24 + 8) * n_contigs
        w["total"] = w["drop_call"]
        w["removed_snps"], w["removed_cells"], w["dropped_reads"] = res["n_removed_snps"], res["n_removed_cells"], res["n_dropped_reads"]
        return w, batch

    res = {"A": [], "B": []}
    for run in range(n_runs + 1):                          # run 0 warms up both routes (allocations) and checks that they agree
        wa, ba, arena, out = route_a()
        wb, bb = route_b()
        if run == 0:
            for c in (0, n_contigs // 2, n_contigs - 1):
                p = out[c]
                ua = lib.ResidentContig(ctx, handle=lib.C.c_void_p(ba._arr[c]), n_reads=p.n_reads)
                ub = lib.ResidentContig(ctx, handle=lib.C.c_void_p(bb._arr[c]), n_reads=p.n_reads)
                for f, cnt in (("read_off", p.n_reads + 1), ("first", p.n_reads), ("last", p.n_reads), ("snp", p.n_cells), ("cell_aw", p.n_cells), ("tw", 2 * p.n_reads), ("meta", 8 * p.n_reads)):
                    assert np.array_equal(ua.download(f, cnt), ub.download(f, cnt)), (c, f)
                ua._h = None; ub._h = None
            print("routes agree on contigs 0, middle, last (all seven fields)", flush=True)
        else:
            res["A"].append(wa); res["B"].append(wb)
        print(f"run {run}: A {wa['total'] * 1e3:.1f} ms  B {wb['total'] * 1e3:.1f} ms", flush=True)
        print("  A", wa, flush=True); print("  B", wb, flush=True)
        ba.free(); arena.free(); bb.free()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for r in ("A", "B"):
        ks = [k for k, v in res[r][0].items() if isinstance(v, float)]
        print(r, "median of", n_runs, ":", {k: round(med([w[k] for w in res[r]]) * 1e3, 2) for k in ks}, "ms; bytes h2d", res[r][0]["h2d_bytes"], "d2h", res[r][0]["d2h_bytes"], flush=True)
    tb = [w["drop_timing"] for w in res["B"]]
    split = {k: round(med([t[k] for t in tb]), 3) for k in ("pileup_ms", "clear_ms", "count_ms", "decide_ms", "filter_count_ms", "filter_fill_ms", "order_ms", "h2d_ms", "d2h_ms", "total_ms")}
    print("B device ms (median):", split, "| count pass / pileup_ms = %.2f" % (split["count_ms"] / max(split["pileup_ms"], 1e-9)), flush=True)
    for c in src:
        c.free()
    ctx.close()


if __name__ == "__main__":
    main()
