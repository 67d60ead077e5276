"""floria-hip on a metagenome-shaped synthetic data set: stage times of the batched flow against one contig per device batch.

    python scripts/cli_timing.py [--contigs 60] [--scale 0.5] [--threads 16] [--sub-rate 0.12] [--realign exact|block:STEP,RULE,TIE ...] [--exe PATH] [--only batched]

--realign (repeatable, needs --only or takes the batched run): the batched run once per scoring, in the order given, e.g. --realign exact --realign block:8,max,right
--pileup-compare N [--threads-list 16,1]: only the batched flow, --pileup host, device, fused and resident ALTERNATING, N runs each per thread count, then the
median and the spread (min .. max) of the ingest time and of the wall time per route, and per route the medians of what the driver reports about its device calls
(profiles/pileup_device.md, profiles/pileup_fused.md, profiles/pileup_resident.md).
--haplosets-compare N [--pileup-route host|resident]: only the batched flow on that --pileup route, --haplosets host and resident ALTERNATING, N runs each, then
the median and the spread (min .. max) of the S2 stage, the COV/ERR/HAPQ stage, their sum and the wall time per setting (profiles/haplosets_resident.md).
--paths-compare N [--pileup-route host|resident]: only the batched flow on that --pileup route under --haplosets resident, --paths host and resident ALTERNATING,
N runs each, then the median and the spread of the phasing stage (upload + S1 + graph: where the read lists come down or do not), the LP + paths stage, the S2 stage,
their sum and the wall time per setting (profiles/paths_resident.md).
--config K --epsilon X --block-length N: the data set's synth configuration (4 = long reads [default], 3 = paired short reads) and the run's -e / -l, e.g.
--config 3 --epsilon 0.04 --block-length 500 for the paired set in the reference arithmetic.
--index-compare N [--parent-exe PATH]: the data set with a .bai written by synth_bam.write_bai beside one copy of the BAM and none beside the other; N runs each,
ALTERNATING, of (a) this build on the copy without an index against --parent-exe (a build of the parent commit) on the same file, (b) -G with the last three contigs
through the index against --no-index, (c) no -G with a VCF thinned to 40 SNPs for every other contig (every contig of this set has the same number of SNPs, so that is
what lets --snp-count-filter 50 drop half of them) through the index against --no-index; then median and spread of the wall time, of the seconds BamStream spent
opening the file (the "BAM header" figure) and of its inflate + decode seconds, and the inflated-member counts (profiles/bam_index.md).
--inflate-compare N [--threads-list 16,1] [--with-index] [--inflate-extra "--no-index"] [--parent-exe PATH]: only the batched flow under --pileup resident,
--inflate host and --inflate device ALTERNATING, N runs each per thread count, one process per run; then median and spread (min .. max) of the ingest seconds, of
BamStream's seconds (inflate + decode on the host route; member planning, inflate, record table on the device route) and of the wall time, and the device route's
report line of its last run.  --with-index writes a .bai beside the BAM; --inflate-extra adds options to every run (e.g. "--no-index" or "--output-reads").  With
--parent-exe the UNFLAGGED tool (--pileup resident alone) of this build also alternates with the parent commit's on the same file (profiles/inflate_route.md).
--estimate-compare N [--threads-list 16,1] [--parent-tree DIR]: only the batched flow under --pileup resident --inflate device WITHOUT -e / -l, --estimate host and
--estimate device ALTERNATING, N runs each per thread count, one process per run; then median and spread (min .. max) of the seconds of the estimate's pass on both
routes (the "BAM header + parameter estimate" figure: opening the file and the pass), of the ingest seconds and of the wall time, and the device route's report line of
its last run (segments, calls, the calls' upload / kernel / download seconds from floria_hip_last_timing).  The run's `Estimated` line must be the same on both routes.
With --parent-tree (the parent commit's tree with library and driver built) the UNFLAGGED tool (--pileup resident alone, -e / -l given) of this build also alternates
with the parent's, and so does bench.py --steps 5 --warmup 2 of the two trees (profiles/estimate_device.md).
--realign exact: the noisy-reads run's realignment under the exact DP beside a fixed-block walk's.  --exe: another build's floria-hip (a previous commit's, for an A/B).

Writes BAM / VCF / FASTA under $TMPDIR, runs the driver twice and prints its stage-time lines (stderr of floria-hip)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from floria_amd import synth, synth_bam  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=60)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=min(32, os.cpu_count() or 1))
    ap.add_argument("--sub-rate", type=float, default=0.0, help="substitution errors in the reads (what realign has to absorb)")
    ap.add_argument("--realign", action="append", default=[], help="run the batched flow once per given scoring (exact | block:STEP,RULE,TIE), in this order")
    ap.add_argument("--exe", default=None, help="floria-hip binary to time (default: this tree's, built first)")
    ap.add_argument("--only", default=None, help="only the runs whose label contains this text")
    ap.add_argument("--arith-compare", action="store_true", help="only: the batched flow at -e 0.04 with --arith canonical against --arith reference (the default there)")
    ap.add_argument("--pileup-compare", type=int, default=0, help="only: the batched flow with --pileup host, device and fused alternating, this many runs each")
    ap.add_argument("--threads-list", default=None, help="with --pileup-compare: comma-separated -t values (default: --threads)")
    ap.add_argument("--haplosets-compare", type=int, default=0, help="only: the batched flow with --haplosets host and resident alternating, this many runs each")
    ap.add_argument("--paths-compare", type=int, default=0, help="only: the batched flow under --haplosets resident with --paths host and resident alternating, this many runs each")
    ap.add_argument("--pileup-route", default="host", help="with --haplosets-compare / --paths-compare: the --pileup route of every run")
    ap.add_argument("--index-compare", type=int, default=0, help="only: indexed against unindexed reading of the BAM, and this build against --parent-exe, this many runs each")
    ap.add_argument("--parent-exe", default=None, help="with --index-compare: floria-hip of the parent commit (comparison (a); left out when not given)")
    ap.add_argument("--inflate-compare", type=int, default=0, help="only: --pileup resident with --inflate host and --inflate device alternating, this many runs each")
    ap.add_argument("--with-index", action="store_true", help="with --inflate-compare: write a .bai beside the BAM")
    ap.add_argument("--inflate-extra", default="", help="with --inflate-compare: further options of every run, space-separated")
    ap.add_argument("--estimate-compare", type=int, default=0, help="only: --pileup resident --inflate device without -e / -l, --estimate host and device alternating, this many runs each")
    ap.add_argument("--parent-tree", default=None, help="with --estimate-compare: the parent commit's tree, built (the unflagged tool and bench.py alternate with this tree's)")
    ap.add_argument("--config", type=int, default=4, help="synth configuration of the contigs (4: long reads, 3: paired short reads)")
    ap.add_argument("--epsilon", default="0.03125", help="-e of every run")
    ap.add_argument("--block-length", default="10000", help="-l of every run")
    a = ap.parse_args()
    if a.exe is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "floria_amd", "host"), "floria-hip"], stdout=subprocess.DEVNULL)
    exe = a.exe or os.path.join(ROOT, "floria_amd", "host", "floria-hip")
    tmp = tempfile.mkdtemp(prefix="floria_cli_")
    prefix = os.path.join(tmp, "d")
    t = time.time()
    cs = [synth.make_config_contig(a.config, i, a.scale, keep_layout=True) for i in range(a.contigs)]
    synth_bam.write_dataset(prefix, cs, seed=1, realign=False, sub_rate=a.sub_rate, index=a.with_index)
    print(f"data set: {a.contigs} contigs, {sum(c.pileup.n_reads for c in cs)} reads, {sum(len(c.snp_pos) for c in cs)} SNPs, "
          f"BAM {os.path.getsize(prefix + '.bam') >> 20} MiB, written in {time.time() - t:.1f}s; host cores {os.cpu_count()}", flush=True)
    if a.index_compare:
        return index_compare(a, exe, tmp, prefix, cs)
    if a.inflate_compare:
        return inflate_compare(a, exe, tmp, prefix)
    if a.estimate_compare:
        return estimate_compare(a, exe, tmp, prefix)
    base = [exe, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-e", a.epsilon, "-l", a.block_length, "--snp-count-filter", "50"]
    runs = (("batched", ["-t", str(a.threads)]), ("batched, 1 thread", ["-t", "1"]), ("one contig per batch", ["-t", str(a.threads), "--batch-contigs", "1"]),
            ("ingest only: realign DP on the host", ["-t", str(a.threads), "--ingest-only"]), ("ingest only, 1 thread", ["-t", "1", "--ingest-only"]))
    if a.arith_compare:
        base[base.index("-e") + 1] = "0.04"
        runs = (("e 0.04, canonical arithmetic", ["-t", str(a.threads), "--arith", "canonical"]), ("e 0.04, reference arithmetic", ["-t", str(a.threads), "--arith", "reference"]),
                ("e 0.04, canonical arithmetic (again)", ["-t", str(a.threads), "--arith", "canonical"]), ("e 0.04, reference arithmetic (again)", ["-t", str(a.threads), "--arith", "reference"]))
    if a.realign:
        runs = tuple((f"batched, --realign {spec}" + (" (again)" if spec in a.realign[:k] else ""), ["-t", str(a.threads), "--realign", spec]) for k, spec in enumerate(a.realign))
    if a.pileup_compare:
        threads = [int(x) for x in a.threads_list.split(",")] if a.threads_list else [a.threads]
        runs = tuple((f"-t {t}, --pileup {route}, run {k + 1}", ["-t", str(t), "--pileup", route]) for t in threads for k in range(a.pileup_compare) for route in ("host", "device", "fused", "resident"))
    if a.haplosets_compare:
        runs = tuple((f"--pileup {a.pileup_route}, --haplosets {h}, run {k + 1}", ["-t", str(a.threads), "--pileup", a.pileup_route, "--haplosets", h])
                     for k in range(a.haplosets_compare) for h in ("host", "resident"))
    if a.paths_compare:
        runs = tuple((f"--pileup {a.pileup_route}, --paths {h}, run {k + 1}", ["-t", str(a.threads), "--pileup", a.pileup_route, "--haplosets", "resident", "--paths", h])
                     for k in range(a.paths_compare) for h in ("host", "resident"))
    if a.only:
        runs = tuple(r for r in runs if a.only in r[0])
    stages = {}
    stats, calls, paths = {}, {}, {}
    for label, extra in runs:
        out = os.path.join(tmp, "o_" + label.replace(" ", "_").replace(",", ""))
        t = time.time()
        r = subprocess.run(base + ["-o", out] + extra, capture_output=True, text=True)
        wall = time.time() - t
        if r.returncode:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith(("Batches", "Total time", "Preprocessing:", "[read_bam]", "Realignment:", "Pileup on the device:", "Resident contigs:", "Haplosets:", "Paths:"))]
        print(f"[{label}] wall {wall:.2f}s | " + " | ".join(lines), flush=True)
        if a.haplosets_compare:
            m = re.search(r"S2 ([\d.]+)s, COV/ERR/HAPQ ([\d.]+)s", next(ln for ln in lines if ln.startswith("Batches")))
            s2, st = float(m.group(1)), float(m.group(2))
            stages.setdefault(label.rsplit(", run", 1)[0], []).append((s2, st, s2 + st, wall))
        if a.paths_compare:
            m = re.search(r"phasing \(upload \+ S1 \+ graph\) ([\d.]+)s, LP \+ paths ([\d.]+)s, S2 ([\d.]+)s", next(ln for ln in lines if ln.startswith("Batches")))
            ph, lp, s2 = float(m.group(1)), float(m.group(2)), float(m.group(3))
            paths.setdefault(label.rsplit(", run", 1)[0], []).append((ph, lp, s2, ph + lp + s2, wall))
        if a.pileup_compare:
            ingest = float(next(ln for ln in lines if ln.startswith("Batches")).split("ingest ")[1].split("s")[0])
            stats.setdefault(label.rsplit(", run", 1)[0], []).append((ingest, wall))
            # what the driver says about its device calls: the pileup call's wall seconds, event seconds and blob bytes; the resident stages' event seconds and bytes back
            pl = next((ln for ln in lines if ln.startswith("Pileup on the device:")), None)
            rs = next((ln for ln in lines if ln.startswith("Resident contigs:")), None)
            d = {}
            if pl:
                m = re.search(r"(\d+) blob bytes in (\d+) calls, ([\d.]+)s .*upload ([\d.]+)s, kernels ([\d.]+)s, download ([\d.]+)s", pl)
                d.update(blob_bytes_up=float(m.group(1)), pileup_calls=float(m.group(2)), pileup_wall_s=float(m.group(3)), pileup_upload_ev_s=float(m.group(4)),
                         pileup_kernels_ev_s=float(m.group(5)), pileup_download_ev_s=float(m.group(6)))
            if rs:
                m = re.search(r"in ([\d.]+)s \(device events ([\d.]+)s\), --ignore-monomorphic filter ([\d.]+)s \(device events ([\d.]+)s.*\); (\d+) bytes came back", rs)
                d.update(assemble_wall_s=float(m.group(1)), assemble_ev_s=float(m.group(2)), filter_wall_s=float(m.group(3)), filter_ev_s=float(m.group(4)), bytes_back=float(m.group(5)))
            calls.setdefault(label.rsplit(", run", 1)[0], []).append(d)
    for key, v in stats.items():
        for k, what in enumerate(("ingest", "wall")):
            x = sorted(t[k] for t in v)
            print(f"[{key}] {what}: median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}s, min {x[0]:.3f}s, max {x[-1]:.3f}s over {len(x)} runs")
    for key, v in stages.items():
        for k, what in enumerate(("S2", "COV/ERR/HAPQ", "S2 + COV/ERR/HAPQ", "wall")):
            x = sorted(t[k] for t in v)
            print(f"[{key}] {what}: median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}s, min {x[0]:.3f}s, max {x[-1]:.3f}s over {len(x)} runs")
    for key, v in paths.items():
        for k, what in enumerate(("phasing", "LP + paths", "S2", "phasing + LP + paths + S2", "wall")):
            x = sorted(t[k] for t in v)
            print(f"[{key}] {what}: median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}s, min {x[0]:.3f}s, max {x[-1]:.3f}s over {len(x)} runs")
    for key, v in calls.items():
        if v and v[0]:
            med = lambda xs: sorted(xs)[len(xs) // 2]
            print(f"[{key}] device calls (medians): " + ", ".join(f"{k} {med([d[k] for d in v]):g}" for k in v[0]))


def inflate_compare(a, exe, tmp, prefix):
    threads = [int(x) for x in a.threads_list.split(",")] if a.threads_list else [a.threads]
    extra = a.inflate_extra.split()

    def cmd(binary, t, more):
        return [binary, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-e", a.epsilon, "-l", a.block_length, "--snp-count-filter", "50", "-t", str(t),
                "--pileup", "resident", *extra, *more]
    for t in threads:
        settings = [("--inflate host", cmd(exe, t, ["--inflate", "host"])), ("--inflate device", cmd(exe, t, ["--inflate", "device"]))]
        if a.parent_exe:
            settings += [("unflagged, this build", cmd(exe, t, [])), ("unflagged, parent build", cmd(a.parent_exe, t, []))]
        got = {label: [] for label, _ in settings}
        last_line = None
        for k in range(a.inflate_compare):
            for label, c in settings:
                out = os.path.join(tmp, "o_inflate")
                t0 = time.time()
                r = subprocess.run(c + ["-o", out], capture_output=True, text=True)
                wall = time.time() - t0
                if r.returncode:
                    print(r.stderr[-2000:])
                    raise SystemExit(1)
                ingest = float(re.search(r"Batches \d+; ingest ([\d.]+)s", r.stderr).group(1))
                stream = float(re.search(r"BAM: \d+ records in \d+ segments, ([\d.]+)s of inflate", r.stderr).group(1))
                got[label].append((ingest, stream, ingest + stream, wall))
                line = next((ln for ln in r.stderr.splitlines() if ln.startswith("Inflate on the device:")), None)
                print(f"[-t {t}, {label}, run {k + 1}] wall {wall:.2f}s, ingest {ingest:.3f}s, BamStream {stream:.3f}s" + (f" | {line}" if line else ""), flush=True)
                last_line = line or last_line
                subprocess.run(["rm", "-rf", out])
        for label, _ in settings:
            for k, what in enumerate(("ingest", "BamStream", "BamStream + ingest", "wall")):
                x = sorted(v[k] for v in got[label])
                print(f"[-t {t}] [{label}] {what}: median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}s, min {x[0]:.3f}s, max {x[-1]:.3f}s over {len(x)} runs", flush=True)
        if last_line:
            print(f"[-t {t}] [--inflate device] last run: {last_line}", flush=True)


def spread(x):
    x = sorted(x)
    return f"median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}, min {x[0]:.3f}, max {x[-1]:.3f} over {len(x)} runs"


def estimate_compare(a, exe, tmp, prefix):
    import json
    threads = [int(x) for x in a.threads_list.split(",")] if a.threads_list else [a.threads]
    files = ["-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "--snp-count-filter", "50"]
    parent_exe = os.path.join(a.parent_tree, "floria_amd", "host", "floria-hip") if a.parent_tree else None
    for t in threads:
        settings = [(f"--estimate {e}", [exe, *files, "-t", str(t), "--pileup", "resident", "--inflate", "device", "--estimate", e]) for e in ("host", "device")]
        if parent_exe:
            settings += [(f"unflagged, {which} build", [binary, *files, "-e", a.epsilon, "-l", a.block_length, "-t", str(t), "--pileup", "resident"])
                         for which, binary in (("this", exe), ("parent", parent_exe))]
        got = {label: [] for label, _ in settings}
        estimated, last_line = {}, None
        for k in range(a.estimate_compare):
            for label, c in settings:
                out = os.path.join(tmp, "o_estimate")
                t0 = time.time()
                r = subprocess.run(c + ["-o", out], capture_output=True, text=True)
                wall = time.time() - t0
                if r.returncode:
                    print(r.stderr[-2000:])
                    raise SystemExit(1)
                ingest = float(re.search(r"Batches \d+; ingest ([\d.]+)s", r.stderr).group(1))
                opened = float(re.search(r"Preprocessing: BAM header[^,]*? ([\d.]+)s,", r.stderr).group(1))
                got[label].append((opened, ingest, wall))
                m = re.search(r"Estimated -l \d+, -e \S+", r.stderr)
                if m:
                    estimated[label] = m.group(0)
                line = next((ln for ln in r.stderr.splitlines() if ln.startswith("Estimate on the device:")), None)
                print(f"[-t {t}, {label}, run {k + 1}] wall {wall:.2f}s, BAM header (+ estimate) {opened:.3f}s, ingest {ingest:.3f}s" + (f" | {line}" if line else ""), flush=True)
                last_line = line or last_line
                subprocess.run(["rm", "-rf", out])
        for label, _ in settings:
            for k, what in enumerate(("BAM header (+ estimate) s", "ingest s", "wall s")):
                print(f"[-t {t}] [{label}] {what}: " + spread([v[k] for v in got[label]]), flush=True)
        print(f"[-t {t}] estimates: {estimated}" + ("" if len(set(estimated.values())) == 1 else "  <-- THE ROUTES DISAGREE"), flush=True)
        if last_line:
            print(f"[-t {t}] [--estimate device] last run: {last_line}", flush=True)
    if a.parent_tree:
        rates = {"this": [], "parent": []}
        for k in range(a.estimate_compare):
            for which, tree in (("this", ROOT), ("parent", os.path.abspath(a.parent_tree))):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], cwd=tree, capture_output=True, text=True)
                if r.returncode:
                    print(r.stdout[-2000:], r.stderr[-3000:])
                    raise SystemExit(1)
                j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                print(f"[bench, {which} tree, run {k + 1}] {j['value']} {j['unit']}", flush=True)
                rates[which].append(float(j["value"]))
        for which, v in rates.items():
            print(f"[bench, {which} tree] " + spread(v), flush=True)


def index_compare(a, exe, tmp, prefix, cs):
    t = time.time()
    indexed = os.path.join(tmp, "dx")                     # the same BAM under a second name, with an index beside it
    os.symlink(prefix + ".bam", indexed + ".bam")
    synth_bam.write_bai(prefix + ".bam", indexed + ".bam.bai")
    thin = prefix + ".thin.vcf"                           # every other contig keeps 40 SNPs: --snp-count-filter 50 drops it
    odd = {c.name for c in cs[1::2]}
    seen = {}
    with open(prefix + ".vcf") as f, open(thin, "w") as g:
        for ln in f:
            name = ln.split("\t", 1)[0]
            if ln.startswith("#") or name not in odd:
                g.write(ln)
            else:
                seen[name] = seen.get(name, 0) + 1
                if seen[name] <= 40:
                    g.write(ln)
    print(f"index written and VCF thinned in {time.time() - t:.1f}s; index {os.path.getsize(indexed + '.bam.bai')} bytes", flush=True)
    last3 = [c.name for c in cs[-3:]]

    def cmd(binary, bam, vcf, extra):
        return [binary, "-b", bam + ".bam", "-v", vcf, "-r", prefix + ".fa", "-e", a.epsilon, "-l", a.block_length, "--snp-count-filter", "50", "-t", str(a.threads),
                "--pileup", a.pileup_route, *extra]
    groups = []
    if a.parent_exe:
        groups.append(("(a) no index", (("this build", cmd(exe, prefix, prefix + ".vcf", [])), ("parent build", cmd(a.parent_exe, prefix, prefix + ".vcf", [])))))
    groups.append(("(b) -G last three contigs", (("indexed", cmd(exe, indexed, prefix + ".vcf", ["-G", *last3])), ("--no-index", cmd(exe, indexed, prefix + ".vcf", ["--no-index", "-G", *last3])))))
    groups.append(("(c) half the contigs under --snp-count-filter", (("indexed", cmd(exe, indexed, thin, [])), ("--no-index", cmd(exe, indexed, thin, ["--no-index"])))))
    for title, pair in groups:
        got = {label: [] for label, _ in pair}
        members = {}
        for k in range(a.index_compare):
            for label, c in pair:
                out = os.path.join(tmp, f"o_ix_{len(got[label])}_{label.replace(' ', '_')}")
                t = time.time()
                r = subprocess.run(c + ["-o", out], capture_output=True, text=True)
                wall = time.time() - t
                if r.returncode:
                    print(r.stderr[-2000:])
                    raise SystemExit(1)
                opened = float(re.search(r"Preprocessing: BAM header\S* ([\d.]+)s", r.stderr).group(1))
                stream = float(re.search(r"BAM: \d+ records in \d+ segments, ([\d.]+)s of inflate", r.stderr).group(1))
                got[label].append((wall, opened, stream, opened + stream))
                m = re.search(r"BAM index \S+: (\d+) targets selected, (\d+) BGZF members inflated for them of (\d+) in the file", r.stderr)
                if m:
                    members[label] = m.groups()
                subprocess.run(["rm", "-rf", out])
        for label, _ in pair:
            for k, what in enumerate(("wall", "BamStream open", "BamStream inflate + decode", "BamStream open + inflate + decode")):
                x = sorted(t[k] for t in got[label])
                print(f"[{title}] [{label}] {what}: median {x[len(x) // 2] if len(x) % 2 else (x[len(x) // 2 - 1] + x[len(x) // 2]) / 2:.3f}s, min {x[0]:.3f}s, max {x[-1]:.3f}s over {len(x)} runs", flush=True)
            if label in members:
                print(f"[{title}] [{label}] targets selected {members[label][0]}, BGZF members inflated {members[label][1]} of {members[label][2]}", flush=True)


if __name__ == "__main__":
    main()
