"""`-m gpu`: floria-hip writes the same files whether it reads the BAM through the .bai beside it or streams it whole (--no-index): -G with two contigs on
the host route and on the resident chain with --output-reads, and a run without -G in which --snp-count-filter does the skipping.  One small long-read set
(eight contigs, 4-KiB BGZF members, index by synth_bam.write_bai) at epsilon = 0.03125."""
import os
import re
import subprocess

import pytest

from floria_amd import synth, synth_bam
from tests.test_gpu_cli import tree_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
REPORT = re.compile(r"BAM index \S+: (\d+) targets selected, (\d+) BGZF members inflated for them of (\d+) in the file")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


@pytest.fixture(scope="module")
def indexed_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_index")
    cs = [synth.make_config_contig(4, 30 + i, 0.05 + 0.015 * i, keep_layout=True) for i in range(8)]           # 25 to 78 SNPs, 120 to 380 reads
    prefix = str(d / "set")
    synth_bam.write_dataset(prefix, cs, seed=5, realign=False, index=True, block_bytes=4096)                   # (realign: only the returned pileups, unused here)
    return prefix, cs


def pair(floria_hip, prefix, tmp_path, extra):
    """the same command with the index and with --no-index -> (tree with, tree without, stderr with)"""
    trees, errs = [], []
    for k, ix in enumerate(((), ("--no-index",))):
        out = str(tmp_path / f"o{k}")
        r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", out, "-e", "0.03125", "-l", "5000", "-t", "4", *extra, *ix],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        trees.append(tree_bytes(out)); errs.append(r.stderr)
    assert REPORT.search(errs[0]) and not REPORT.search(errs[1])
    reads = lambda e: [ln for ln in e.splitlines() if ln.startswith("Number of reads passing filtering")]
    assert reads(errs[0]) == reads(errs[1])
    return trees[0], trees[1], errs[0]


def same_trees(a, b, n_contigs):
    assert sorted(a) == sorted(b)
    assert len([n for n in a if n.endswith(".vartigs")]) == n_contigs
    for n in a:
        assert a[n] == b[n], n


@pytest.mark.parametrize("route", [("--pileup", "host"), ("--pileup", "resident", "--paths", "resident", "--output-reads")], ids=["host", "resident_chain"])
def test_two_named_contigs_give_the_same_files_through_the_index(floria_hip, indexed_set, tmp_path, route):
    prefix, cs = indexed_set
    a, b, err = pair(floria_hip, prefix, tmp_path, ("-G", cs[6].name, cs[2].name, "--snp-count-filter", "10", *route))
    same_trees(a, b, 2)
    rows = a["contig_ploidy_info.tsv"].decode().splitlines()
    assert [r.split("\t")[0] for r in rows[1:]] == [cs[2].name, cs[6].name]             # header order, whatever the order of -G
    m = REPORT.search(err)
    assert int(m.group(1)) == 2 and 0 < int(m.group(2)) < int(m.group(3))


def test_snp_count_filter_selects_the_contigs_the_index_reads(floria_hip, indexed_set, tmp_path):
    prefix, cs = indexed_set
    counts = sorted(len(c.snp_pos) for c in cs)
    cut = counts[4]                                                                      # the four contigs with the fewest SNPs are dropped
    assert counts[3] < cut
    keep = [c.name for c in cs if len(c.snp_pos) >= cut]
    a, b, err = pair(floria_hip, prefix, tmp_path, ("--snp-count-filter", str(cut), "--ignore-monomorphic"))
    same_trees(a, b, len(keep))
    rows = a["contig_ploidy_info.tsv"].decode().splitlines()
    assert [r.split("\t")[0] for r in rows[1:]] == keep
    m = REPORT.search(err)
    assert int(m.group(1)) == len(keep) and 0 < int(m.group(2)) < int(m.group(3))
    assert err.count("This warning will not be shown from now on") == 1
