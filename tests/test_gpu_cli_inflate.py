"""`-m gpu`: floria-hip --pileup resident --inflate device against --pileup resident on the same inputs: the same files byte for byte and the same resident arrays
behind every contig's handle (--dump-handles), at -e 0.03125 and at -e 0.04.  Every case also reads the route's report line ("Inflate on the device: ..."), so that
none passes by missing what it is about: several segments, carried-over members, a segment that ends at a gap, bytes that came down for a host-walk contig or a
CG-tag record."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import plan_model as plm
from tests.test_gpu_cli_resident import (EPS, HAND, NINE, edited, floria_hip, hand, merged_dataset, nine, noisy, paired, parse_handles,  # noqa: F401 (fixtures)
                                         run_resident)
from tests.test_gpu_pileup import hand_built

pytestmark = pytest.mark.gpu

REPORT = re.compile(r"Inflate on the device: (\d+) segments, (\d+) BGZF members sent \((\d+) compressed bytes up, (\d+) inflated bytes on the device\), (\d+) segments re-planned "
                    r"for look-ahead, (\d+) members re-inflated as carry-over, (\d+) bytes down for host use \((\d+) for host-walk contigs, (\d+) for CG records\); "
                    r"inflate ([0-9.]+)s, record table ([0-9.]+)s, sequences ([0-9.]+)s")
FIELDS = ("segments", "members", "compressed", "inflated", "replanned", "carried", "down", "down_host_walk", "down_cg")


def report(err):
    m = REPORT.search(err)
    assert m, err
    return dict(zip(FIELDS, map(int, m.groups()[:9])))


def inflate_agrees(floria_hip, tmp_path, prefix, extra=(), eps_list=EPS, seq_pos=False, min_files=4):
    """--pileup resident without and with --inflate device, into the SAME output directory one after the other -> [(host-inflate stderr, device stderr, report)]"""
    out = []
    for eps in eps_list:
        o = str(tmp_path / "out")
        hh, dh, hs, ds = (str(tmp_path / n) for n in ("handles_host.txt", "handles_device.txt", "seqpos_host.txt", "seqpos_device.txt"))
        sp = lambda f: ("--dump-seq-pos", f) if seq_pos else ()
        host_tree, host_err = run_resident(floria_hip, prefix, o, eps, (*extra, "--dump-handles", hh, *sp(hs)))
        dev_tree, dev_err = run_resident(floria_hip, prefix, o, eps, (*extra, "--inflate", "device", "--dump-handles", dh, *sp(ds)))
        assert "Inflate on the device:" not in host_err
        rep = report(dev_err)
        assert rep["segments"] >= 1 and rep["members"] >= 1 and rep["inflated"] > rep["compressed"] > 0
        assert sorted(dev_tree) == sorted(host_tree) and len(host_tree) >= min_files, (sorted(dev_tree), sorted(host_tree))
        for fn in host_tree:
            assert dev_tree[fn] == host_tree[fn], f"{fn} differs at -e {eps}"
        assert parse_handles(hh) == parse_handles(dh), f"the handles differ at -e {eps}"
        if seq_pos:
            assert open(hs).read() == open(ds).read() and os.path.getsize(hs) > 1000, f"--dump-seq-pos differs at -e {eps}"
        reads = lambda err: re.findall(r"Number of reads passing filtering: \d+ \(\S+\)", err)
        assert reads(dev_err) == reads(host_err)
        out.append((host_err, dev_err, rep))
    return out


# ---- one contig ----------------------------------------------------------------------------------------------------------------------------------------
def test_noisy_long_reads_with_the_exact_dp(floria_hip, tmp_path, noisy):
    for host_err, dev_err, rep in inflate_agrees(floria_hip, tmp_path, noisy):
        line = lambda err: re.search(r"Realignment: \d+ calls scored on the device behind the walk \([^)]*\)", err).group(0)
        assert line(dev_err) == line(host_err) and rep["down"] == 0


def test_noisy_long_reads_without_realignment(floria_hip, tmp_path, noisy):
    inflate_agrees(floria_hip, tmp_path, noisy, extra=("--no-realign",))


def test_paired_short_reads_on_derived_set_orders(floria_hip, tmp_path, paired):
    res = inflate_agrees(floria_hip, tmp_path, paired, extra=("-l", "500"))
    assert "derived on the device" in res[1][1] and "derived on the device" not in res[0][1]


@pytest.fixture(scope="module")
def hand_n(tmp_path_factory):
    """the hand-built supplementary / hard-clip set with the case records, and two reads of this file's own: one of ODD length with an N base (on a SNP and off one),
    and one of one base more, so that an odd and an even record stand side by side in the blob"""
    prefix = str(tmp_path_factory.mktemp("hand_n") / "h")
    hand_built(prefix)
    plm.add_case_records(prefix)
    targets, records = plm.read_bam(prefix + ".bam")
    ref = np.frombuffer("".join(l.strip() for l in open(prefix + ".fa") if not l.startswith(">")).encode(), np.uint8)
    rows = [(r["pos"], r["raw"]) for r in records]
    for name, at, n in (("x_odd_n", 4800, 4501), ("x_even_n", 4810, 4502)):
        s = ref[at:at + n].copy()
        s[7] = ord("N")
        s[5000 - at] = ord("N")                                   # (SNPs stand at 1000 + 500 k)
        s[n - 1] = ord("N")                                       # the last base: the nibble whose partner is padding in the odd read
        rows.append((at, synth_bam.bam_record(0, at, name, 0, 60, [("M", n)], bytes(s), (np.arange(n) % 41).astype(np.uint8))))
    rows.sort(key=lambda t: t[0])
    synth_bam.write_bam(prefix + ".bam", targets, [raw for _, raw in rows])
    return prefix


@pytest.mark.parametrize("trim", [(), ("--extra-trimming",)])
def test_supplementary_and_hard_clipped_set_with_output_reads(floria_hip, tmp_path, hand_n, trim):
    res = inflate_agrees(floria_hip, tmp_path, hand_n, extra=(*HAND, "--output-reads", *trim), seq_pos=True, min_files=6)
    fastq = b"".join(open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(tmp_path / "out") for f in fs if f.endswith(".fastq"))
    assert b"x_odd_n" in fastq and b"x_even_n" in fastq and b"supp_near" in fastq and b"N" not in fastq.split(b"x_odd_n")[1].split(b"\n")[1]
    assert all(rep["down"] == 0 for _, _, rep in res)


@pytest.mark.parametrize("which", ["noisy", "hand"])
def test_ignore_monomorphic(floria_hip, tmp_path, request, which):
    prefix = request.getfixturevalue(which)
    extra = {"noisy": (), "hand": HAND}[which]
    for _, dev_err, _ in inflate_agrees(floria_hip, tmp_path, prefix, extra=(*extra, "--ignore-monomorphic", "--output-reads")):
        m = re.search(r"(\d+) SNPs removed, (\d+) reads dropped", dev_err)
        assert int(m.group(1)) >= 1 and int(m.group(2)) >= 1


# ---- nine contigs -----------------------------------------------------------------------------------------------------------------------------------------
def nine_set(tmp_path_factory, name, **kw):
    cs = [synth.make_config_contig(4, 20 + i, 0.12 + 0.02 * i, keep_layout=True) for i in range(8)] + [synth.make_config_contig(3, 5, 0.1, keep_layout=True)]
    prefix = str(tmp_path_factory.mktemp(name) / "d")
    synth_bam.write_dataset(prefix, cs, seed=7, edit_frac=0.5, **kw)
    return prefix


@pytest.fixture(scope="module")
def nine_indexed(tmp_path_factory):
    return nine_set(tmp_path_factory, "nine_ix", index=True)


@pytest.fixture(scope="module")
def nine_small_members(tmp_path_factory):
    return nine_set(tmp_path_factory, "nine_sm", index=True, block_bytes=1500)


def test_nine_contigs_without_an_index(floria_hip, tmp_path, nine):
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, nine, extra=NINE, min_files=30):
        assert "BAM index" not in dev_err and "Resident contigs: 9 assembled" in dev_err


def test_nine_contigs_through_the_index(floria_hip, tmp_path, nine_indexed):
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, nine_indexed, extra=NINE, min_files=30):
        assert "BAM index" in dev_err and "9 targets selected" in dev_err and rep["carried"] == 0


def test_nine_contigs_with_an_index_that_is_ignored(floria_hip, tmp_path, nine_indexed):
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, nine_indexed, extra=(*NINE, "--no-index"), min_files=30):
        assert "BAM index" not in dev_err


def test_first_and_last_contig_named_so_that_a_segment_ends_at_the_gap(floria_hip, tmp_path, nine_indexed):
    names = [n for n, _ in plm.read_bam(nine_indexed + ".bam")[0]]
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, nine_indexed, extra=(*NINE, "-G", names[0], names[-1]), min_files=6):
        assert "2 targets selected" in dev_err and rep["segments"] >= 2                 # seven contigs lie between the two: their members do not go up
        whole = report(run_resident(floria_hip, nine_indexed, str(tmp_path / "out"), EPS[0], (*NINE, "--inflate", "device"))[1])
        assert rep["compressed"] < whole["compressed"] // 2


@pytest.mark.parametrize("index", [False, True])
def test_small_window_gives_several_segments_and_carried_members(floria_hip, tmp_path, nine, nine_indexed, index):
    prefix = nine_indexed if index else nine
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, prefix, extra=(*NINE, "--bam-window-kb", "64", "-t", "1"), min_files=30):
        assert rep["segments"] > 1
        assert int(re.search(r"Pileup on the device: \d+ records, \d+ blob bytes in (\d+) calls", dev_err).group(1)) > 1
        if not index:
            assert rep["carried"] >= 1                                                   # a streamed segment ends inside a target: its members go up again


@pytest.mark.parametrize("extra", [(), ("--no-index",), ("--bam-window-kb", "64")])
def test_records_that_straddle_members(floria_hip, tmp_path, nine_small_members, extra):
    """members of 1 500 inflated bytes: what the input guarantees is RECORDS CROSSING A MEMBER BOUNDARY - every long read's record is larger than a member - and
    targets that begin inside one; that is checked here before the run is relied on, on the member list synth_bam._bgzf_members reads from the file's member headers
    (the rule of BamStream's own walk, bgzf_member: BSIZE from the BC subfield, ISIZE from the trailer; the tool does not print its list).  (Whether a look-ahead re-plan happens
    depends on where the index's end offsets fall and is not asserted.)"""
    packed = open(nine_small_members + ".bam", "rb").read()
    members, raw = synth_bam._bgzf_members(packed)
    bounds = np.array([o for _, o in members], np.int64)
    _, records = plm.read_bam(nine_small_members + ".bam")
    o = raw.index(records[0]["raw"])
    crossing = 0
    for r in records:
        crossing += int(np.searchsorted(bounds, o, "right") != np.searchsorted(bounds, o + len(r["raw"]) - 1, "right"))
        o += len(r["raw"])
    assert o == len(raw) and crossing > len(records) // 2 and len(members) > 100
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, nine_small_members, extra=(*NINE, *extra), eps_list=EPS[:1], min_files=30):
        assert rep["members"] >= len(members) - 2 and "Resident contigs: 9 assembled" in dev_err


# ---- what still needs the host --------------------------------------------------------------------------------------------------------------------------------
def test_five_allele_contig_in_a_mixed_batch_comes_down_for_the_host_walk(floria_hip, tmp_path, edited):
    five = str(tmp_path / "five")
    hand_built(five, five_alleles=True)
    prefix = str(tmp_path / "m")
    merged_dataset(prefix, [edited, five])
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, prefix, extra=(*HAND, "--no-realign", "--output-reads"), min_files=8):
        assert dev_err.count("keeps the host walk") == 1 and "contig c " in dev_err and "Resident contigs: 1 assembled" in dev_err
        assert rep["down_host_walk"] > 100000 and rep["down"] == rep["down_host_walk"] + rep["down_cg"]


def test_record_whose_cigar_lives_in_the_cg_tag(floria_hip, tmp_path):
    """70 000 operations, 35 000 x (1M 1I) from 9 000 (the record of tests/test_host_cpu.py, rebuilt on the hand-built contig): the field holds the kSmN placeholder,
    the real CIGAR stands in CG:B,I behind other tags.  Its bytes come down once, the tag's place in the blob goes to the walk."""
    prefix = str(tmp_path / "cg")
    hand_built(prefix)
    targets, records = plm.read_bam(prefix + ".bam")
    ref = np.frombuffer("".join(l.strip() for l in open(prefix + ".fa") if not l.startswith(">")).encode(), np.uint8)
    alt = {int(l.split("\t")[1]) - 1: ord(l.split("\t")[4][0]) for l in open(prefix + ".vcf") if not l.startswith("#")}
    at, n = 9000, 35000
    seq = np.full(2 * n, ord("A"), np.uint8)
    seq[0::2] = ref[at:at + n]
    for q, a in alt.items():
        if at <= q < at + n and (q // 500) % 2:
            seq[2 * (q - at)] = a
    rec = synth_bam.bam_record(0, at, "x_cg", 0, 60, [("S", 2 * n), ("N", n)], bytes(seq), np.full(2 * n, 30, np.uint8))
    cigar = b"".join(struct.pack("<II", 1 << 4 | 0, 1 << 4 | 1) for _ in range(n))
    body = rec[4:] + b"XAA!" + b"NMi" + struct.pack("<i", n) + b"XZZtext\0" + b"CGBI" + struct.pack("<I", 2 * n) + cigar
    rows = sorted([(r["pos"], r["raw"]) for r in records] + [(at, struct.pack("<I", len(body)) + body)], key=lambda t: t[0])
    synth_bam.write_bam(prefix + ".bam", targets, [raw for _, raw in rows])
    for _, dev_err, rep in inflate_agrees(floria_hip, tmp_path, prefix, extra=(*HAND, "--output-reads"), seq_pos=True):
        assert rep["down_cg"] == len(body) + 4 and rep["down_host_walk"] == 0
        line = [l for l in open(tmp_path / "seqpos_device.txt") if l.startswith("x_cg\t")]
        assert len(line) == 1 and len(line[0].split("\t")) > 60                         # its SNPs were walked through the real CIGAR: query offset 2 (p - 9 000)
        assert all(int(x.split(":")[2]) == 2 * (1000 + 500 * (int(x.split(":")[0]) - 1) - at) for x in line[0].rstrip("\n").split("\t")[1:])


def test_ingest_only_dump_plan_is_the_host_inflate_routes(floria_hip, tmp_path, hand, paired, nine_indexed):
    for prefix, extra in ((hand, HAND), (paired, ()), (nine_indexed, NINE)):
        plans = {}
        for inflate in ("host", "device"):
            plan = str(tmp_path / f"plan_{inflate}.txt")
            r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.04", "-l", "10000", "-t", "4",
                                "--ingest-only", "--pileup", "resident", "--inflate", inflate, "--dump-plan", plan, *extra], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            plans[inflate] = open(plan).read()
            assert ("Inflate on the device:" in r.stderr) == (inflate == "device") and not os.path.exists(tmp_path / "unused")
        assert plans["host"] == plans["device"] and plans["host"].count("\nF\t") > 200


def test_gzip_file_without_bgzf_members_points_to_inflate_host(floria_hip, tmp_path, hand):
    import gzip
    import shutil
    prefix = str(tmp_path / "g")
    for ext in (".vcf", ".fa"):
        shutil.copy(hand + ext, prefix + ext)
    with open(prefix + ".bam", "wb") as f:
        f.write(gzip.compress(gzip.open(hand + ".bam", "rb").read()))
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "out"), "-e", "0.04", "-l", "10000", "--pileup", "resident",
                        "--inflate", "device", *HAND], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "gzip file without BGZF members" in r.stderr and "--inflate host" in r.stderr
