#!/usr/bin/env python3
"""The driver's ingest seconds (the closing "Batches" line) under --ingest-only --no-realign, this tree's floria-hip against another build of it, alternating.

  python scripts/ingest_ab.py CONFIG CONTIGS SCALE THREADS RUNS OTHER_EXE

CONFIG 4: long reads, 3: paired short reads (floria_amd/synth.py).  Needs no GPU.  Prints every run, then per build the median, min and max, and whether this
tree's median lies inside the other build's min-max range (profiles/host_driver_refactor.md).
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floria_amd import synth, synth_bam  # noqa: E402


def main():
    config, n_contigs, scale, threads, runs, other = int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]), sys.argv[4], int(sys.argv[5]), sys.argv[6]
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "floria_amd", "host"), "floria-hip"], stdout=subprocess.DEVNULL)
    tmp = tempfile.mkdtemp(prefix="floria_ingest_ab_")
    prefix = os.path.join(tmp, "d")
    t = time.time()
    cs = [synth.make_config_contig(config, i, scale, keep_layout=True) for i in range(n_contigs)]
    synth_bam.write_dataset(prefix, cs, seed=1, realign=False)
    print(f"data set: config {config}, {n_contigs} contigs, {sum(c.pileup.n_reads for c in cs)} reads, {sum(len(c.snp_pos) for c in cs)} SNPs, "
          f"BAM {os.path.getsize(prefix + '.bam') >> 20} MiB, written in {time.time() - t:.1f}s; host cores {os.cpu_count()}", flush=True)
    res = {"other": [], "this tree": []}
    for k in range(runs):
        for label, exe in (("other", other), ("this tree", os.path.join(ROOT, "floria_amd", "host", "floria-hip"))):
            r = subprocess.run([exe, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", os.path.join(tmp, "unused"), "-e", "0.03125", "-l", "10000",
                                "--snp-count-filter", "50", "-t", threads, "--ingest-only", "--no-realign"], capture_output=True, text=True)
            if r.returncode:
                print(r.stderr[-2000:])
                raise SystemExit(1)
            res[label].append(float(re.search(r"ingest ([\d.]+)s", r.stderr).group(1)))
            print(f"run {k + 1} {label}: ingest {res[label][-1]:.3f}s", flush=True)
    for label, v in res.items():
        print(f"{label}: median {statistics.median(v):.3f}s, min {min(v):.3f}s, max {max(v):.3f}s")
    print("this tree's median inside the other build's min-max range:", min(res["other"]) <= statistics.median(res["this tree"]) <= max(res["other"]))


if __name__ == "__main__":
    main()
