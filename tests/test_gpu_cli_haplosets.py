"""`-m gpu`: floria-hip --haplosets resident against the default (--haplosets host) on the same inputs: the same files, byte for byte, under --pileup host and
--pileup resident, with --output-reads, at -e 0.04 on paired short reads, and with a batch of one contig."""
import os
import re
import subprocess

import pytest

from floria_amd import synth, synth_bam
from tests.test_gpu_cli_resident import run_resident

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


@pytest.fixture(scope="module")
def three_long(tmp_path_factory):
    cs = [synth.make_config_contig(4, 30 + i, 0.12 + 0.03 * i, keep_layout=True) for i in range(3)]
    prefix = str(tmp_path_factory.mktemp("three") / "d")
    synth_bam.write_dataset(prefix, cs, seed=11, edit_frac=0.5)
    return prefix


@pytest.fixture(scope="module")
def paired_short(tmp_path_factory):
    c = synth.make_config_contig(3, 4, 0.15, keep_layout=True)
    prefix = str(tmp_path_factory.mktemp("paired") / "d")
    synth_bam.write_dataset(prefix, [c], seed=11)
    return prefix


def same_files(floria_hip, tmp_path, prefix, eps, route, extra, min_files=4):
    """both runs write to the SAME output directory one after the other (its path is part of every vartig header)"""
    out = str(tmp_path / "out")
    want, _ = run_resident(floria_hip, prefix, out, eps, extra, route=route)
    got, err = run_resident(floria_hip, prefix, out, eps, (*extra, "--haplosets", "resident"), route=route)
    m = re.search(r"Haplosets: (\d+) split, sorted and kept on the device behind S2", err)
    assert m and int(m.group(1)) >= 2, err                            # the run took the handle's path
    explicit, _ = run_resident(floria_hip, prefix, out, eps, (*extra, "--haplosets", "host"), route=route) if route == "host" and not extra else (want, "")
    assert sorted(got) == sorted(want) == sorted(explicit) and len(want) >= min_files, (sorted(got), sorted(want))
    for fn in want:
        assert got[fn] == want[fn], f"{fn} differs under --pileup {route} {' '.join(extra)}"
        assert explicit[fn] == want[fn], fn
    return want


LONG = ("--snp-count-filter", "50")


@pytest.mark.parametrize("route", ["host", "resident"])
def test_three_long_read_contigs_without_and_with_output_reads(floria_hip, tmp_path, three_long, route):
    plain = same_files(floria_hip, tmp_path, three_long, 0.03125, route, LONG, min_files=10)
    want = same_files(floria_hip, tmp_path, three_long, 0.03125, route, (*LONG, "--output-reads"), min_files=10)
    assert len(want) > len(plain)                                      # the read files are there


def test_batches_of_one_contig(floria_hip, tmp_path, three_long):
    same_files(floria_hip, tmp_path, three_long, 0.03125, "resident", (*LONG, "--batch-contigs", "1", "--output-reads"), min_files=10)
    same_files(floria_hip, tmp_path, three_long, 0.03125, "host", (*LONG, "--batch-contigs", "1"), min_files=10)


@pytest.mark.parametrize("route", ["host", "resident"])
def test_paired_short_reads_in_the_reference_arithmetic(floria_hip, tmp_path, paired_short, route):
    same_files(floria_hip, tmp_path, paired_short, 0.04, route, ("-l", "500", "--output-reads"))
