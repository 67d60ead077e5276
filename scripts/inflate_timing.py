"""BGZF inflate + record table + resident pileup ON THE DEVICE against the host path, at the C ABI (profiles/inflate_device.md).

    python scripts/inflate_timing.py [--contigs 200] [--scale 0.5] [--runs 5] [--parent-tree scripts/tmp_prev] [--window-mb 512] [--no-tool] [--no-bench | --only-bench]

The data set is scripts/cli_timing.py's (synth_bam.write_dataset, seed 1, long reads).  Per run, ALTERNATING, one process each:
  tool     floria-hip --ingest-only --pileup resident at -t 16 and -t 1, of the parent tree and of this one: the BamStream inflate + decode seconds and the
           "Pileup on the device" line (the floria_hip_pileup_records_resident calls with their staged upload)
  host     floria_hip_pileup_records_resident with a HOST blob, per segment of the window, parent tree and this one (the inflated bytes pageable, as BamStream leaves them)
  device   this tree: floria_hip_inflate_bgzf (the file in floria_hip_host_alloc memory), floria_hip_blob_records with one chain per contig and with one chain,
           floria_hip_pileup_records_resident_blob; wall and event times, bytes host -> device and device -> host of each
  bench    python bench.py --steps 5 --warmup 2 of the parent tree and of this one
A segment is a run of consecutive BGZF members whose inflated bytes fit the window; its chains cover the records that lie wholly inside it (the one record a
segment boundary cuts is left out on both paths).  PARENT_TREE is the parent commit's floria_amd/ + include/ + bench.py with library and driver built; it is not
committed.  Every worker warms up with the first segment before it measures."""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def members_of(packed):
    """-> (offset, bytes, isize) of every BGZF member"""
    off, out, n = 0, [], len(packed)
    while off < n:
        xlen, = struct.unpack_from("<H", packed, off + 10)
        x = off + 12
        bsize = None
        while x + 4 <= off + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", packed, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", packed, x + 4)[0] + 1
            x += 4 + slen
        out.append((off, bsize, struct.unpack_from("<I", packed, off + bsize - 4)[0], 12 + xlen))
        off += bsize
    return np.array(out, np.int64)


def inflate_host(packed, mem, pool):
    """the members' inflated bytes back to back, by zlib on `pool`"""
    out = np.empty(int(mem[:, 2].sum()), np.uint8)
    at = np.concatenate([[0], np.cumsum(mem[:, 2])])

    def one(i):
        o, b, isz, h = (int(v) for v in mem[i])
        if isz:
            out[at[i]:at[i] + isz] = np.frombuffer(zlib.decompress(packed[o + h:o + b - 8], -15), np.uint8)
    list(pool.map(one, range(len(mem)), chunksize=64))
    return out


def record_table(raw, start):
    """offsets (of the block_size prefix) and ref_id of every record from `start` on"""
    offs, refs, o, n = [], [], start, len(raw)
    view = memoryview(raw)
    while o + 4 <= n:
        bs, ref = struct.unpack_from("<Ii", view, o)
        if o + 4 + bs > n:
            break
        offs.append(o); refs.append(ref)
        o += 4 + bs
    return np.array(offs, np.int64), np.array(refs, np.int64), o


def prepare(prefix, window, tmp):
    """once: the member table, the segments, and per segment the chains and the record arrays (header-sized) -> an .npz the workers read"""
    packed = open(prefix + ".bam", "rb").read()
    mem = members_of(packed)
    with ThreadPoolExecutor(16) as pool:
        raw = inflate_host(packed, mem, pool)
    l_text, = struct.unpack_from("<I", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, o)
    o += 4
    names = []
    for _ in range(n_ref):
        ln, = struct.unpack_from("<I", raw, o)
        names.append(bytes(raw[o + 4:o + 4 + ln - 1]).decode())
        o += 8 + ln
    offs, refs, _ = record_table(raw, o)
    ends = np.append(offs[1:], len(raw))
    seg_first, acc = [0], 0
    for i, isz in enumerate(mem[:, 2]):
        if acc + isz > window and acc:
            seg_first.append(i); acc = 0
        acc += isz
    seg_first.append(len(mem))
    at = np.concatenate([[0], np.cumsum(mem[:, 2])])
    save = dict(mem=mem, seg_first=np.array(seg_first), names=np.array(names))
    for k in range(len(seg_first) - 1):
        s, e = int(at[seg_first[k]]), int(at[seg_first[k + 1]])
        sel = np.nonzero((offs >= s) & (ends <= e))[0]
        save[f"rec_{k}"] = offs[sel] - s
        save[f"end_{k}"] = ends[sel] - s
        save[f"ref_{k}"] = refs[sel]
    path = os.path.join(tmp, "prepared.npz")
    np.savez(path, **save)
    print(f"prepared: {len(mem)} BGZF members, {len(raw)} inflated bytes, {len(offs)} records, {len(seg_first) - 1} segments of at most {window >> 20} MiB", flush=True)
    return path


def worker(a):
    sys.path.insert(0, a.tree)
    sys.path.insert(1, ROOT)
    from floria_amd import lib
    from tests import pileup_model as pm
    P = np.load(a.prepared)
    mem, seg_first, names = P["mem"], P["seg_first"], [str(x) for x in P["names"]]
    size = os.path.getsize(a.data + ".bam")
    arena = lib.PinnedArena(size + 64)
    packed = arena.take(size, np.uint8)
    with open(a.data + ".bam", "rb") as f:
        f.readinto(memoryview(packed))
    tables = pm.read_vcf_tables(a.data + ".vcf", names)
    tab = pm.pack_tables([tables[n] for n in names])
    seqs, cur = {}, None
    for line in open(a.data + ".fa"):
        if line.startswith(">"):
            cur = line[1:].split()[0]; seqs[cur] = []
        else:
            seqs[cur].append(line.strip())
    ref_off = np.cumsum([0] + [sum(len(x) for x in seqs[n]) for n in names]).astype(np.uint64)
    ref_seq = np.frombuffer("".join("".join(seqs[n]) for n in names).encode(), np.uint8)
    ctx = lib.FloriaHip(0)
    tot = {}

    def add(key, wall, t=None, up=0, down=0):
        d = tot.setdefault(key, dict(wall_s=0.0, h2d_ms=0.0, kernels_ms=0.0, d2h_ms=0.0, bytes_up=0, bytes_down=0))
        d["wall_s"] += wall
        if t:
            d["h2d_ms"] += t["h2d_ms"]; d["kernels_ms"] += t["pileup_ms"]; d["d2h_ms"] += t["d2h_ms"]
            d["bytes_up"] += int(t["upload_pinned_bytes"] + t["upload_staged_bytes"])
        d["bytes_up"] += up; d["bytes_down"] += down

    def rec_args(t):
        cig = t["offset"] + np.uint64(36) + t["l_read_name"].astype(np.uint64)
        seq = cig + np.uint64(4) * t["n_cigar_op"].astype(np.uint64)
        return dict(pos=t["pos"], flags=t["flag"], contig=t["ref_id"].astype(np.uint32), cigar_off=cig, n_cigar=t["n_cigar_op"].astype(np.uint32), seq_off=seq, l_seq=t["l_seq"],
                    qual_off=seq + ((t["l_seq"].astype(np.uint64) + np.uint64(1)) >> np.uint64(1)))
    pool = ThreadPoolExecutor(16)
    cells = 0
    for k in [0] + list(range(len(seg_first) - 1)):                     # the first segment twice: once to warm up
        warm = k == 0 and not tot.get("_warmed")
        m = mem[seg_first[k]:seg_first[k + 1]]
        rec, end, ref = P[f"rec_{k}"], P[f"end_{k}"], P[f"ref_{k}"]
        cut = np.nonzero(np.diff(ref))[0] + 1
        c_begin = rec[np.concatenate([[0], cut])].astype(np.uint64); c_end = end[np.concatenate([cut - 1, [len(rec) - 1]])].astype(np.uint64)
        if a.mode == "host":
            raw = inflate_host(packed, m, pool)
            view = memoryview(raw)
            hdr = np.array([struct.unpack_from("<iiBBHHHI", view, int(o) + 4) for o in rec], np.int64)          # refID pos l_read_name mapq bin n_cigar flag l_seq
            t = dict(offset=rec.astype(np.uint64), ref_id=hdr[:, 0].astype(np.int32), pos=hdr[:, 1].astype(np.int32), l_read_name=hdr[:, 2].astype(np.uint8),
                     n_cigar_op=hdr[:, 5].astype(np.uint16), flag=hdr[:, 6].astype(np.uint16), l_seq=hdr[:, 7].astype(np.uint32))
            t0 = time.perf_counter()
            s = ctx.pileup_records_resident(blob=raw, **rec_args(t), **tab, ref_off=ref_off, ref_seq=ref_seq)
            w = time.perf_counter() - t0
            if not warm:
                add("pileup_records_resident, host blob", w, ctx.timing(), down=24 * len(rec) + 8)
                cells += s.counts["cells"]
            s.free()
        else:
            t0 = time.perf_counter()
            blob = ctx.inflate_bgzf(packed, m[:, 0].astype(np.uint64), m[:, 1].astype(np.uint32))
            w = time.perf_counter() - t0
            if not warm:
                add("inflate_bgzf", w, ctx.timing(), down=4 * len(m))
            t0 = time.perf_counter()
            tb = ctx.blob_records(blob, c_begin, c_end)
            w = time.perf_counter() - t0
            back = sum(v.nbytes for v in tb.values())
            assert np.array_equal(tb["offset"].astype(np.int64), rec)
            if not warm:
                add("blob_records, one chain per contig", w, ctx.timing(), up=16 * len(c_begin), down=back)
            t0 = time.perf_counter()
            t1 = ctx.blob_records(blob, [int(rec[0])], [int(end[-1])])
            w = time.perf_counter() - t0
            assert np.array_equal(t1["offset"], tb["offset"])
            if not warm:
                add("blob_records, one chain", w, ctx.timing(), up=16, down=back)
            t0 = time.perf_counter()
            s = ctx.pileup_records_resident(blob=blob, **rec_args(tb), **tab, ref_off=ref_off, ref_seq=ref_seq)
            w = time.perf_counter() - t0
            if not warm:
                add("pileup_records_resident, blob handle", w, ctx.timing(), down=24 * len(rec) + 8)
                cells += s.counts["cells"]
            s.free()
            blob.free()
        tot["_warmed"] = True
    del tot["_warmed"]
    print("RESULT " + json.dumps(dict(mode=a.mode, tree=a.tree, cells=int(cells), calls=tot)), flush=True)
    ctx.close()


def med(xs):
    x = sorted(xs)
    return f"{x[len(x) // 2]:.3f} ({x[0]:.3f} .. {x[-1]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=200)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--window-mb", type=int, default=512)
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--only-bench", action="store_true", help="the bench.py comparison alone (no data set is written)")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--mode", default="device")
    ap.add_argument("--data", default=None)
    ap.add_argument("--prepared", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    sys.path.insert(0, ROOT)
    from floria_amd import synth, synth_bam
    tmp = tempfile.mkdtemp(prefix="floria_inflate_")
    prefix = os.path.join(tmp, "d")
    t = time.time()
    if a.only_bench:
        a.no_tool, a.contigs = True, 0
    cs = [synth.make_config_contig(4, i, a.scale, keep_layout=True) for i in range(a.contigs)]
    synth_bam.write_dataset(prefix, cs, seed=1, realign=False)
    print(f"data set: {a.contigs} contigs, {sum(c.pileup.n_reads for c in cs)} reads, {sum(len(c.snp_pos) for c in cs)} SNPs, BAM {os.path.getsize(prefix + '.bam') >> 20} MiB, "
          f"written in {time.time() - t:.1f}s", flush=True)
    del cs
    prepared = None if a.only_bench else prepare(prefix, a.window_mb << 20, tmp)
    trees = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("this", ROOT)]
    rows = {}

    def note(key, **kv):
        for k, v in kv.items():
            rows.setdefault((key, k), []).append(v)
    for run in range(a.runs):
        if not a.no_tool:
            for threads in (16, 1):
                for label, tree in trees:
                    exe = os.path.join(tree, "floria_amd", "host", "floria-hip")
                    t0 = time.time()
                    r = subprocess.run([exe, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-e", "0.03125", "-l", "10000", "--snp-count-filter", "50", "-t", str(threads),
                                        "--ingest-only", "--pileup", "resident", "-o", os.path.join(tmp, "o")], capture_output=True, text=True)
                    wall = time.time() - t0
                    if r.returncode:
                        print(r.stderr[-2000:]); raise SystemExit(1)
                    bam = float(re.search(r"([\d.]+)s of inflate \+ decode", r.stderr).group(1))
                    m = re.search(r"Pileup on the device: \d+ records, (\d+) blob bytes in (\d+) calls, ([\d.]+)s .*upload ([\d.]+)s, kernels ([\d.]+)s, download ([\d.]+)s", r.stderr)
                    print(f"[run {run + 1}] tool, {label}, -t {threads}: wall {wall:.2f}s, BamStream inflate + decode {bam:.3f}s, pileup calls {m.group(3)}s of which upload {m.group(4)}s, "
                          f"kernels {m.group(5)}s, download {m.group(6)}s; {m.group(1)} blob bytes in {m.group(2)} calls", flush=True)
                    note(f"tool, {label}, -t {threads}", wall=wall, bamstream=bam, pileup_calls=float(m.group(3)), upload=float(m.group(4)), kernels=float(m.group(5)))
        for label, tree, mode in [] if a.only_bench else [(lb, tr, "host") for lb, tr in trees] + [("this", ROOT, "device")]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--mode", mode, "--data", prefix, "--prepared", prepared], capture_output=True, text=True)
            if r.returncode:
                print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
            res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
            for call, d in res["calls"].items():
                print(f"[run {run + 1}] ABI, {label}: {call}: wall {d['wall_s']:.3f}s, h2d {d['h2d_ms'] / 1e3:.3f}s, kernels {d['kernels_ms'] / 1e3:.3f}s, d2h {d['d2h_ms'] / 1e3:.3f}s, "
                      f"{d['bytes_up']} bytes up, {d['bytes_down']} bytes down; {res['cells']} cells", flush=True)
                note(f"ABI, {label}: {call}", wall=d["wall_s"], h2d=d["h2d_ms"] / 1e3, kernels=d["kernels_ms"] / 1e3)
        if not a.no_bench:
            for label, tree in trees:
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], cwd=tree, capture_output=True, text=True)
                if r.returncode:
                    print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
                j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                print(f"[run {run + 1}] bench, {label}: {j['value']} {j['unit']}, {j['ms_per_step']} ms per step", flush=True)
                note(f"bench, {label}", blocks_per_s=j["value"])
    for (key, what), v in rows.items():
        print(f"{key} | {what}: median {med(v)} over {len(v)} runs")


if __name__ == "__main__":
    main()
