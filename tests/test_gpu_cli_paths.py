"""`-m gpu`: floria-hip --paths resident against the default (--paths host) on the same inputs: the same files, byte for byte — long reads and paired short reads, at
-e 0.03125 and 0.04, under --pileup host and --pileup resident, with --debug (debug_graph.txt prints the nodes' reads and the paths' reads), --output-reads and
--ignore-monomorphic, in batches of three contigs, and on two contexts of one device.  Under --paths resident S1 returns no read list (unless --debug), the path
peeling returns node lists, and one floria_hip_join_paths + one floria_hip_reassign_haplosets_resident call per batch replace the host's union and the list upload."""
import os
import re
import shutil
import subprocess

import pytest

from floria_amd import synth, synth_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


@pytest.fixture(scope="module")
def long_reads(tmp_path_factory):
    contigs = [synth.make_config_contig(4, i, 0.5, keep_layout=True) for i in range(5)]
    prefix = str(tmp_path_factory.mktemp("long") / "d")
    synth_bam.write_dataset(prefix, contigs, seed=7)
    return prefix


@pytest.fixture(scope="module")
def paired(tmp_path_factory):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path_factory.mktemp("paired") / "d")
    synth_bam.write_dataset(prefix, [c], seed=7)
    return prefix


def run(floria_hip, prefix, out, eps, extra):
    if os.path.exists(out):
        shutil.rmtree(out)
    cmd = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", out, "-e", repr(eps), "-l", "10000", "-t", "4", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    tree = {}
    for dp, _, fs in os.walk(out):
        for f in fs:
            if f != "cmd.log":
                tree[os.path.relpath(os.path.join(dp, f), out)] = open(os.path.join(dp, f), "rb").read()
    return tree, r.stderr, open(os.path.join(out, "cmd.log")).read()


def routes_agree(floria_hip, tmp_path, prefix, eps, extra=(), min_files=4, debug=False):
    """both routes write to the SAME output directory one after the other (its path is part of every vartig header)"""
    out = str(tmp_path / "out")
    host_tree, host_err, _ = run(floria_hip, prefix, out, eps, extra)
    res_tree, res_err, cmd = run(floria_hip, prefix, out, eps, (*extra, "--paths", "resident"))
    assert "--paths resident" in cmd and "Paths: --paths resident" not in host_err
    m = re.search(r"Paths: --paths resident: (\d+) hap-graph paths joined into haplosets on the device", res_err)
    assert m and int(m.group(1)) > 0, res_err
    assert ("returned its read lists" if debug else "returned no read list") in res_err
    assert "Haplosets: " in res_err                                            # --paths resident implies --haplosets resident
    assert sorted(res_tree) == sorted(host_tree) and len(host_tree) >= min_files, (sorted(res_tree), sorted(host_tree))
    for fn in host_tree:
        assert res_tree[fn] == host_tree[fn], f"{fn} differs at -e {eps}"
    return host_tree


@pytest.mark.parametrize("eps", [0.03125, 0.04])
@pytest.mark.parametrize("pileup", ["host", "resident"])
def test_long_reads(floria_hip, tmp_path, long_reads, pileup, eps):
    tree = routes_agree(floria_hip, tmp_path, long_reads, eps, ("--pileup", pileup), min_files=10)
    assert sum(fn.endswith(".haplosets") and len(v) > 100 for fn, v in tree.items()) == 5


@pytest.mark.parametrize("eps", [0.03125, 0.04])
@pytest.mark.parametrize("pileup", ["host", "resident"])
def test_paired_short_reads(floria_hip, tmp_path, paired, pileup, eps):
    routes_agree(floria_hip, tmp_path, paired, eps, ("--pileup", pileup))


@pytest.mark.parametrize("pileup", ["host", "resident"])
def test_debug_output_reads_and_ignore_monomorphic(floria_hip, tmp_path, long_reads, pileup):
    tree = routes_agree(floria_hip, tmp_path, long_reads, 0.04, ("--pileup", pileup, "--debug", "--output-reads", "--ignore-monomorphic"), min_files=10, debug=True)
    graphs = [v for fn, v in tree.items() if fn.endswith("debug_graph.txt")]
    assert len(graphs) == 5 and all(b"\nP\t" in g and g.startswith(b"N\t") for g in graphs)
    assert any("long_reads" in fn and fn.endswith(".fastq") for fn in tree)


def test_batches_of_three_contigs(floria_hip, tmp_path, long_reads):
    routes_agree(floria_hip, tmp_path, long_reads, 0.04, ("--pileup", "resident", "--batch-contigs", "3"), min_files=10)
    routes_agree(floria_hip, tmp_path, long_reads, 0.03125, ("--batch-contigs", "3"), min_files=10)


def test_two_contexts_on_one_device(floria_hip, tmp_path, long_reads):
    routes_agree(floria_hip, tmp_path, long_reads, 0.04, ("--pileup", "host", "--devices", "0,0"), min_files=10)
