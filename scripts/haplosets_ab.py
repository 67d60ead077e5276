"""ABI-level A/B of the stretch between S2 and the writers, on the batch bench.py's `pipeline` leg uses (the first 250 contigs of a BASELINE configuration):

    host arrays : floria_hip_reassign_batch + floria_hip_haploset_stats + floria_hip_hapq_batch + floria_hip_haploset_alleles on the returned lists
    by handle   : floria_hip_reassign_batch_resident + floria_hip_haplosets_download + the three consumers by handle

    python scripts/haplosets_ab.py [--contigs 250] [--config 4] [--scale 1.0] [--runs 5] [--epsilon 0.03125]

The two alternate, --runs times each after one warm-up pair; every C entry point is called with arrays prepared outside the timed region (for the host-array path
the concatenation of the returned lists is INSIDE it: that marshalling is what a host pays between the calls; it is done in numpy, one concatenate per array).
Prints per run the wall ms of the S2 call, of the consumers and of the whole, the device-event span of the S2 call (floria_timing.total_ms) and the bytes each
way, then median and min .. max per path.  floria_hip_read_spans needs contigs that carry positions, which uploads do not: its leg is measured inside the tool
(scripts/cli_timing.py --haplosets-compare --pileup-route resident)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from floria_amd import _capi as capi, lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=250)
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.03125)
    a = ap.parse_args()
    lib.build()
    L = lib.load()
    cfg = synth.CONFIGS[a.config]
    contigs = [synth.make_config_contig(a.config, i, a.scale) for i in range(a.contigs)]
    ctx = lib.FloriaHip(0)
    handles = ctx.upload_batch([c.pileup for c in contigs])
    n = len(handles)
    arr = (C.c_void_p * n)(*[h._h for h in handles])
    bc, bs, be = [], [], []
    for j, c in enumerate(contigs):
        s, e = lib.get_range_with_lengths(c.snp_pos, cfg["block_length"])
        bc += [j] * len(s); bs += list(s); be += list(e)
    r = ctx.phase_blocks_batch(handles, bc, bs, be, lib.make_params(a.epsilon, cfg["max_ploidy"], cfg["beam"]))
    gc, groups, ranges = [], [], []
    for b in range(r.n_blocks):
        for part in r.partitions(b):
            if len(part):
                groups.append(part); ranges.append((int(bs[b]), int(be[b]))); gc.append(int(bc[b]))
    gc = np.ascontiguousarray(gc, np.uint32)
    off = np.zeros(len(groups) + 1, np.uint64); off[1:] = np.cumsum([len(g) for g in groups])
    reads = np.ascontiguousarray(np.concatenate(groups), np.uint32)
    rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
    pos = [np.ascontiguousarray(c.snp_pos, np.uint64) for c in contigs]
    pp = (C.POINTER(C.c_uint64) * n)(*[capi.ptr(p, C.c_uint64) for p in pos])
    ns = np.ascontiguousarray([len(p) for p in pos], np.uint32)
    p32, p64, pf = (lambda x: capi.ptr(x, C.c_uint32)), (lambda x: capi.ptr(x, C.c_uint64)), (lambda x: capi.ptr(x, C.c_double))
    print(f"batch: {n} contigs of config {a.config} (scale {a.scale}), {sum(c.pileup.n_reads for c in contigs)} reads, {len(groups)} haplosets into S2, {len(reads)} read ids", flush=True)

    def consumers_out(ng, rg):
        lens = np.maximum(0, rg[1::2].astype(np.int64) - rg[0::2].astype(np.int64) + 1)
        pos_off = np.zeros(ng + 1, np.uint64); pos_off[1:] = np.cumsum(lens)
        return (np.zeros((ng, 4), np.float64), np.zeros(ng, np.uint8), np.zeros(ng, np.float64), np.zeros(n, np.float64), pos_off, np.zeros((int(pos_off[-1]), 4), np.uint32))

    def by_arrays():
        t0 = time.perf_counter()
        out = C.POINTER(C.POINTER(capi.CGroups))()
        lib._check(L.floria_hip_reassign_batch(ctx._h, arr, n, p32(gc), p64(off), p32(reads), p32(rng), len(groups), None, None, C.c_double(a.epsilon), C.byref(out)))
        ev = ctx.timing()["total_ms"]
        t1 = time.perf_counter()
        # what a host does with the result before the next call: the final lists as one set of arrays again
        gs = [out[i].contents for i in range(n)]
        fng = np.array([g.n_groups for g in gs], np.int64)
        fgc = np.repeat(np.arange(n, dtype=np.uint32), fng)
        offs = [np.ctypeslib.as_array(g.grp_off, shape=(g.n_groups + 1,)) for g in gs]
        tot = np.array([int(o[-1]) for o in offs], np.uint64)
        base = np.concatenate([[0], np.cumsum(tot)]).astype(np.uint64)
        foff = np.concatenate([o[:-1] + base[i] for i, o in enumerate(offs)] + [base[-1:]]).astype(np.uint64)
        frd = np.concatenate([np.ctypeslib.as_array(g.grp_read, shape=(max(1, int(tot[i])),))[:int(tot[i])] for i, g in enumerate(gs)]).astype(np.uint32)
        frg = np.concatenate([np.ctypeslib.as_array(g.range, shape=(max(1, 2 * g.n_groups),))[:2 * g.n_groups] for g in gs]).astype(np.uint32)
        ng = int(fng.sum())
        st, hq, rel, avg, pos_off, cnt = consumers_out(ng, frg)
        t2 = time.perf_counter()
        lib._check(L.floria_hip_haploset_stats(ctx._h, arr, n, p32(fgc), p64(foff), p32(frd), p32(frg), ng, pf(st)))
        lib._check(L.floria_hip_hapq_batch(ctx._h, arr, n, p32(fgc), p64(foff), p32(frd), p32(frg), ng, pp, p32(ns), C.c_uint64(cfg["block_length"]), capi.ptr(hq, C.c_uint8), pf(rel), pf(avg)))
        lib._check(L.floria_hip_haploset_alleles(ctx._h, arr, n, p32(fgc), p64(foff), p32(frd), p32(frg), ng, p64(pos_off), p32(cnt)))
        t3 = time.perf_counter()
        L.floria_hip_groups_array_free(out, n)
        lists = 4 * len(fgc) + 8 * len(foff) + 4 * len(frd) + 4 * len(frg)
        up = 4 * len(gc) + 8 * len(off) + 4 * len(reads) + 4 * len(rng) + 3 * lists + 8 * len(foff) * 2
        down = 4 * sum(c.pileup.n_reads for c in contigs) + st.nbytes + cnt.nbytes
        return dict(s2_ms=(t1 - t0) * 1e3, marshal_ms=(t2 - t1) * 1e3, consumers_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3, s2_event_ms=ev, bytes_up=up, bytes_down=down), (st, hq, rel, avg, cnt, frd, frg)

    def by_handle():
        t0 = time.perf_counter()
        h = C.c_void_p()
        lib._check(L.floria_hip_reassign_batch_resident(ctx._h, arr, n, p32(gc), p64(off), p32(reads), p32(rng), len(groups), None, None, C.c_double(a.epsilon), C.byref(h)))
        ev = ctx.timing()["total_ms"]
        out = C.POINTER(C.POINTER(capi.CGroups))()
        lib._check(L.floria_hip_haplosets_download(h, C.byref(out)))
        t1 = time.perf_counter()
        gs = [out[i].contents for i in range(n)]
        frg = np.concatenate([np.ctypeslib.as_array(g.range, shape=(max(1, 2 * g.n_groups),))[:2 * g.n_groups] for g in gs]).astype(np.uint32)   # pos_off is the caller's
        ng = len(frg) // 2
        st, hq, rel, avg, pos_off, cnt = consumers_out(ng, frg)
        t2 = time.perf_counter()
        lib._check(L.floria_hip_haploset_stats_resident(ctx._h, arr, n, h, pf(st)))
        lib._check(L.floria_hip_hapq_batch_resident(ctx._h, arr, n, h, pp, p32(ns), C.c_uint64(cfg["block_length"]), capi.ptr(hq, C.c_uint8), pf(rel), pf(avg)))
        lib._check(L.floria_hip_haploset_alleles_resident(ctx._h, arr, n, h, p64(pos_off), p32(cnt)))
        t3 = time.perf_counter()
        tot = sum(int(np.ctypeslib.as_array(g.grp_off, shape=(g.n_groups + 1,))[-1]) for g in gs)
        frd = np.concatenate([np.ctypeslib.as_array(g.grp_read, shape=(max(1, int(np.ctypeslib.as_array(g.grp_off, shape=(g.n_groups + 1,))[-1])),))[:int(np.ctypeslib.as_array(g.grp_off, shape=(g.n_groups + 1,))[-1])] for g in gs]).astype(np.uint32)
        L.floria_hip_groups_array_free(out, n)
        L.floria_hip_haplosets_free(h)
        up = 4 * len(gc) + 8 * len(off) + 4 * len(reads) + 4 * len(rng) + 20 * len(groups) + 8 * (ng + 1) * 2
        down = 16 * n + (8 * (ng + 1) + 8 * ng) + 4 * tot + 8 * ng + st.nbytes + cnt.nbytes
        return dict(s2_ms=(t1 - t0) * 1e3, marshal_ms=(t2 - t1) * 1e3, consumers_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3, s2_event_ms=ev, bytes_up=up, bytes_down=down), (st, hq, rel, avg, cnt, frd, frg)

    (_, ra), (_, rb) = by_arrays(), by_handle()                      # warm-up pair, and the two paths agree bit for bit
    for x, y in zip(ra, rb):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the two paths differ"
    rows = {"host arrays": [], "by handle": []}
    for k in range(a.runs):
        for name, f in (("host arrays", by_arrays), ("by handle", by_handle)):
            m, _ = f()
            rows[name].append(m)
            print(f"run {k + 1} [{name}] " + ", ".join(f"{key} {v:.3f}" if isinstance(v, float) else f"{key} {v}" for key, v in m.items()), flush=True)
    for name, v in rows.items():
        for key in ("s2_ms", "marshal_ms", "consumers_ms", "total_ms", "s2_event_ms"):
            x = sorted(m[key] for m in v)
            print(f"[{name}] {key}: median {x[len(x) // 2]:.3f}, min {x[0]:.3f}, max {x[-1]:.3f} over {len(x)} runs")
    for h in handles:
        h.free()
    ctx.close()


if __name__ == "__main__":
    main()
