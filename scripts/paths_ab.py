"""ABI-level A/B of the stretch from S1 to S2's result, on the batch bench.py's `pipeline` leg uses (the first 250 contigs of a BASELINE configuration):

    lists on the host : floria_hip_phase_blocks_batch (read lists come back), floria_hip_hap_graph, the nodes' read sets from the lists (what build_columns does),
                        the union per path, floria_hip_reassign_batch_resident on the united lists
    by handle         : the same S1 call under "s1_no_lists" = 1, floria_hip_hap_graph, floria_hip_join_paths, floria_hip_reassign_haplosets_resident

    python scripts/paths_ab.py [--contigs 250] [--config 4] [--scale 1.0] [--runs 5] [--epsilon 0.03125]

No LP runs here.  The paths are the same fixed node lists in both variants, made once from a first S1 call: path k of a contig takes partition k of every block of
the contig that has one (a chain through the whole contig, as the peeled paths of a long-read contig are); what the host decides between the hap graph and the join
is not part of either stretch.  The host side of the first variant is numpy (one stable sort of the lists by (block, partition), one unique per path): it stands
for build_columns + the union of the C++ host, which walk the same 5 B per (block, read) with push_back loops.
The two alternate, --runs times each after a warm-up pair that also checks that both return the same haplosets.  Prints per run the wall ms of every step and the
bytes each way (from the array sizes), then median and min .. max per variant."""
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
    bc, bs, be = (np.ascontiguousarray(x, np.uint32) for x in (bc, bs, be))
    nb = len(bc)
    prm = lib.make_params(a.epsilon, cfg["max_ploidy"], cfg["beam"])
    p32, p64 = (lambda x: capi.ptr(x, C.c_uint32)), (lambda x: capi.ptr(x, C.c_uint64))

    def s1(no_lists):
        ctx.set_option("s1_no_lists", 1 if no_lists else 0)
        out = C.POINTER(capi.CBlockResult)()
        try:
            lib._check(L.floria_hip_phase_blocks_batch(ctx._h, arr, n, p32(bc), p32(bs), p32(be), nb, C.byref(prm), C.byref(out)))
        finally:
            ctx.set_option("s1_no_lists", 0)
        return out

    def graph(res):
        g = C.POINTER(capi.CHapGraph)()
        lib._check(L.floria_hip_hap_graph(ctx._h, res, C.byref(g)))
        L.floria_hip_hap_graph_free(g)

    # the fixed paths, from a first call
    r0 = s1(False)
    bp = capi.np_from(r0.contents.best_ploidy, nb, np.uint32)
    L.floria_hip_block_result_free(r0)
    path_contig, node_off, node_block, node_part, path_range = [], [0], [], [], []
    for j in range(n):
        blocks = np.nonzero(bc == j)[0]
        for k in range(int(bp[blocks].max()) if len(blocks) else 0):
            mine = blocks[bp[blocks] > k]
            node_block += mine.tolist(); node_part += [k] * len(mine)
            path_contig.append(j); node_off.append(len(node_block)); path_range += [int(bs[mine].min()), int(be[mine].max())]
    path_contig, node_block, path_range = (np.ascontiguousarray(x, np.uint32) for x in (path_contig, node_block, path_range))
    node_off, node_part = np.ascontiguousarray(node_off, np.uint64), np.ascontiguousarray(node_part, np.uint8)
    n_paths, n_nodes = len(path_contig), len(node_block)
    node_key = node_block.astype(np.int64) * 16 + node_part

    def download(h):
        out = C.POINTER(C.POINTER(capi.CGroups))()
        lib._check(L.floria_hip_haplosets_download(h, C.byref(out)))
        gs = [capi.Groups(out[i].contents) for i in range(n)]
        L.floria_hip_groups_array_free(out, n)
        return gs

    def on_the_host():
        t0 = time.perf_counter()
        res = s1(False)
        t1 = time.perf_counter()
        graph(res)
        t2 = time.perf_counter()
        c = res.contents
        tot = int(c.read_off[nb])
        ro = np.ctypeslib.as_array(c.read_off, shape=(nb + 1,)).astype(np.int64)
        ids = np.ctypeslib.as_array(c.read_id, shape=(tot,)); part = np.ctypeslib.as_array(c.part, shape=(tot,))
        key = np.repeat(np.arange(nb, dtype=np.int64), np.diff(ro)) * 16 + part            # the nodes' read sets: the lists grouped by (block, partition)
        order = np.argsort(key, kind="stable")
        by_node, skey = ids[order], key[order]
        lo, hi = np.searchsorted(skey, node_key, "left"), np.searchsorted(skey, node_key, "right")
        t3 = time.perf_counter()
        groups = [np.unique(np.concatenate([by_node[lo[x]:hi[x]] for x in range(int(node_off[p]), int(node_off[p + 1]))])) for p in range(n_paths)]      # the union per path
        off = np.zeros(n_paths + 1, np.uint64); off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate(groups), np.uint32)
        t4 = time.perf_counter()
        h = C.c_void_p()
        lib._check(L.floria_hip_reassign_batch_resident(ctx._h, arr, n, p32(path_contig), p64(off), p32(reads), p32(path_range), n_paths, None, None, C.c_double(a.epsilon), C.byref(h)))
        t5 = time.perf_counter()
        L.floria_hip_block_result_free(res)
        down = 5 * tot + 16 * n
        up = 4 * len(reads) + 8 * len(off) + 12 * n_paths
        return dict(s1_ms=(t1 - t0) * 1e3, graph_ms=(t2 - t1) * 1e3, nodes_ms=(t3 - t2) * 1e3, union_ms=(t4 - t3) * 1e3, s2_ms=(t5 - t4) * 1e3, total_ms=(t5 - t0) * 1e3,
                    bytes_up=up, bytes_down=down), h

    def by_handle():
        t0 = time.perf_counter()
        res = s1(True)
        t1 = time.perf_counter()
        graph(res)
        t2 = time.perf_counter()
        j = C.c_void_p()
        lib._check(L.floria_hip_join_paths(ctx._h, res, arr, n, p32(path_contig), p64(node_off), p32(node_block), capi.ptr(node_part, C.c_uint8), p32(path_range), n_paths, C.byref(j)))
        t4 = time.perf_counter()
        h = C.c_void_p()
        lib._check(L.floria_hip_reassign_haplosets_resident(ctx._h, arr, n, j, C.c_double(a.epsilon), C.byref(h)))
        t5 = time.perf_counter()
        L.floria_hip_haplosets_free(j)
        L.floria_hip_block_result_free(res)
        down = 8 + 16 * n + 24 * n_paths + 8 * n_paths + 8 * (n + 1) + 16 * n            # bitmap size, counts, the join handle's header mirror and spans, multi counts, counts
        up = 13 * n_nodes + 8 * (n_paths + 1) + 12 * n_paths
        return dict(s1_ms=(t1 - t0) * 1e3, graph_ms=(t2 - t1) * 1e3, nodes_ms=0.0, union_ms=(t4 - t2) * 1e3, s2_ms=(t5 - t4) * 1e3, total_ms=(t5 - t0) * 1e3,
                    bytes_up=up, bytes_down=down), h

    (_, ha), (_, hb) = on_the_host(), by_handle()                      # warm-up pair, and the two variants agree list for list
    for x, y in zip(download(ha), download(hb)):
        assert np.array_equal(x.grp_off, y.grp_off) and np.array_equal(x.grp_read, y.grp_read) and np.array_equal(x.range, y.range), "the two variants differ"
    L.floria_hip_haplosets_free(ha); L.floria_hip_haplosets_free(hb)
    print(f"batch: {n} contigs of config {a.config} (scale {a.scale}), {sum(c.pileup.n_reads for c in contigs)} reads, {nb} blocks, {n_paths} paths of {n_nodes} nodes", flush=True)
    rows = {"lists on the host": [], "by handle": []}
    for k in range(a.runs):
        for name, f in (("lists on the host", on_the_host), ("by handle", by_handle)):
            m, h = f()
            L.floria_hip_haplosets_free(h)
            rows[name].append(m)
            print(f"run {k + 1} [{name}] " + ", ".join(f"{key} {v:.3f}" if isinstance(v, float) else f"{key} {v}" for key, v in m.items()), flush=True)
    for name, v in rows.items():
        for key in ("s1_ms", "graph_ms", "nodes_ms", "union_ms", "s2_ms", "total_ms"):
            x = sorted(m[key] for m in v)
            print(f"[{name}] {key}: median {x[len(x) // 2]:.3f}, min {x[0]:.3f}, max {x[-1]:.3f} over {len(x)} runs")
    for h in handles:
        h.free()
    ctx.close()


if __name__ == "__main__":
    main()
