"""`-m "not gpu"`: floria-hip reads only the contigs it will phase when a .bai lies beside the BAM.  The BAM is written here: eight targets of 20 to 60 long
reads in 512-byte BGZF members (records straddle members, targets begin inside one), target 3 without a read, targets 5 and 6 with fewer SNPs than
--snp-count-filter 20, and an unplaced tail.  tests/bai_model.py says, from the BAM alone, where every target begins and which members hold its records;
synth_bam.write_bai and the reader in ingest.cpp are both held against it.  Every run gives -e and -l, so no estimate pass reads the file."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from floria_amd import synth_bam
from tests import bai_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
N_READS = [40, 20, 60, 0, 35, 25, 30, 45]
N_SNPS = [40, 40, 40, 40, 40, 10, 10, 40]                 # targets 5 and 6 fall to --snp-count-filter 20
NAMES = [f"ctg{t}" for t in range(8)]
CONTIG_LEN = 9000
REPORT = re.compile(r"BAM index (\S+): (\d+) targets selected, (\d+) BGZF members inflated for them of (\d+) in the file")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def write_set(prefix, unplaced=30, block_bytes=512):
    """{prefix}.bam / .vcf / .fa of the set above (no index)"""
    rng = np.random.default_rng(11)
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    recs = []
    with open(prefix + ".fa", "w") as fa, open(prefix + ".vcf", "w") as vcf:
        vcf.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for t, name in enumerate(NAMES):
            ref = "".join("ACGT"[i] for i in rng.integers(0, 4, size=CONTIG_LEN))
            fa.write(f">{name}\n{ref}\n")
            snps = [300 + 200 * i for i in range(N_SNPS[t])]
            for q in snps:
                vcf.write(f"{name}\t{q + 1}\t.\t{ref[q]}\t{nxt[ref[q]]}\t50\tPASS\tDP=10\n")
            for r in range(N_READS[t]):
                beg = (CONTIG_LEN - 900) * r // N_READS[t]
                ln = 500 + 37 * (r % 9)
                s = list(ref[beg:beg + ln])
                for q in snps:
                    if beg <= q < beg + ln and (r + q // 200) % 2 == 0:
                        s[q - beg] = nxt[ref[q]]
                recs.append(synth_bam.bam_record(t, beg, f"{name}_r{r}", 0, 60, [("M", ln)], "".join(s).encode(), np.full(ln, 30, np.uint8)))
    for r in range(unplaced):
        recs.append(synth_bam.bam_record(-1, -1, f"u{r}", 4, 0, [], b"ACGTACGTAC" * 10, np.full(100, 20, np.uint8)))
    synth_bam.write_bam(prefix + ".bam", [(n, CONTIG_LEN) for n in NAMES], recs, block_bytes=block_bytes)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the set twice: `ix` with x.bam.bai beside it, `plain` without an index; and the model of the BAM (the two BAMs are the same bytes)"""
    d = tmp_path_factory.mktemp("bai")
    ix, plain = str(d / "ix"), str(d / "plain")
    write_set(ix)
    for ext in (".bam", ".vcf", ".fa"):
        shutil.copyfile(ix + ext, plain + ext)
    synth_bam.write_bai(ix + ".bam")
    return dict(dir=d, ix=ix, plain=plain, model=bai_model.model(ix + ".bam"))


def copy_set(data, tmp_path, name, index_bytes=None, index_name=None):
    """a copy of the set under tmp_path, with the given bytes as its index (default: none)"""
    prefix = str(tmp_path / name)
    for ext in (".bam", ".vcf", ".fa"):
        shutil.copyfile(data["ix"] + ext, prefix + ext)
    if index_bytes is not None:
        with open(index_name or prefix + ".bam.bai", "wb") as f:
            f.write(index_bytes)
    return prefix


def run(floria_hip, prefix, tmp_path, extra=(), ok=True):
    """--ingest-only --pileup host --dump-frags -> (dump text, stderr, return code)"""
    dump = str(tmp_path / "frags.txt")
    if os.path.exists(dump):
        os.remove(dump)
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "out"), "-e", "0.03125", "-l", "2000",
                        "--ingest-only", "--pileup", "host", "--dump-frags", dump, "--snp-count-filter", "20", "-t", "3", *extra], capture_output=True, text=True, timeout=120)
    if ok:
        assert r.returncode == 0, r.stderr
    return (open(dump).read() if os.path.exists(dump) else ""), r.stderr, r.returncode


def selected(names=None):
    """the targets a run phases: those -G names (all without -G) that have enough SNPs"""
    return [t for t in range(8) if (names is None or NAMES[t] in names) and N_SNPS[t] >= 20]


def test_the_set_is_what_the_tests_need(data):
    m = data["model"]
    assert m["names"] == NAMES and m["n_unplaced"] == 30
    assert [m["n_records"].get(t, 0) for t in range(8)] == N_READS
    assert m["n_members"] > 300
    # targets begin inside a member, and consecutive targets share their boundary member
    assert sum(1 for t in m["begin"] if m["begin"][t] & 0xffff) >= 6
    assert m["members"][0] & m["members"][1]


@pytest.mark.parametrize("pseudo_bin", [True, False])
def test_write_bai_begins_equal_the_model(data, tmp_path, pseudo_bin):
    m = data["model"]
    bai = synth_bam.write_bai(data["ix"] + ".bam", str(tmp_path / "w.bai"), pseudo_bin=pseudo_bin)
    begins, pseudo, n_ref = bai_model.bai_begins(bai)
    assert n_ref == 8
    assert begins == m["begin"] and 3 not in begins
    assert pseudo == (m["begin"] if pseudo_bin else {})
    raw = open(bai, "rb").read()
    assert struct.unpack_from("<Q", raw, len(raw) - 8)[0] == 30                 # n_no_coor


def test_samtools_index_gives_the_same_begins(data, tmp_path):
    m = data["model"]
    ours, _, _ = bai_model.bai_begins(data["ix"] + ".bam.bai")
    assert ours == m["begin"]
    samtools = shutil.which("samtools")
    if samtools:                                                                  # (absent: no index of another program has been read)
        bam = str(tmp_path / "s.bam")
        shutil.copyfile(data["ix"] + ".bam", bam)
        subprocess.check_call([samtools, "index", bam], timeout=120)
        theirs, _, _ = bai_model.bai_begins(bam + ".bai")
        assert theirs == m["begin"]


CASES = {
    "all": None,
    "first": ["ctg0"],
    "last": ["ctg7"],
    "empty": ["ctg3"],
    "adjacent": ["ctg1", "ctg2"],
    "far_apart": ["ctg0", "ctg7"],
    "reverse_order": ["ctg7", "ctg4", "ctg2", "ctg0"],
    "with_unknown_name": ["ctg2", "no_such_contig"],
    "filtered_only": ["ctg5", "ctg6"],
}


@pytest.mark.parametrize("window", [(), ("--bam-window-kb", "1"), ("--bam-window-kb", "64")], ids=["window_default", "window_1k", "window_64k"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_same_frags_with_the_index_and_fewer_members(floria_hip, data, tmp_path, case, window):
    names = CASES[case]
    g = () if names is None else ("-G", *names)
    want, err0, _ = run(floria_hip, data["ix"], tmp_path, extra=("--no-index", *g, *window))
    got, err1, _ = run(floria_hip, data["ix"], tmp_path, extra=(*g, *window))
    assert got == want
    sel = selected(names)
    assert [ln.split("\t")[1] for ln in got.splitlines() if ln.startswith("#CONTIG")] == [NAMES[t] for t in sel if N_READS[t]]
    reads = lambda err: [ln for ln in err.splitlines() if ln.startswith("Number of reads passing filtering")]
    assert reads(err1) == reads(err0) and len(reads(err1)) == len(sel)
    warned = lambda err: [ln for ln in err.splitlines() if "variants. This warning" in ln]
    assert warned(err1) == warned(err0)
    # the report: only with the index; no read can be had with fewer members than the model's union, and one look-ahead per stretch is all that is spent on top
    assert not REPORT.search(err0)
    rep = REPORT.search(err1)
    assert rep, err1
    m = data["model"]
    union = set().union(*[m["members"].get(t, set()) for t in sel]) if sel else set()
    n_sel, inflated, in_file = int(rep.group(2)), int(rep.group(3)), int(rep.group(4))
    assert rep.group(1) == data["ix"] + ".bam.bai"
    assert n_sel == len(sel) and in_file == m["n_members"]
    assert len(union) <= inflated <= len(union) + len(sel)
    if case == "last":
        assert 0 < inflated < in_file
    if case in ("empty", "filtered_only"):
        assert inflated == 0
    segs = lambda err: int(re.search(r"BAM: \d+ records in (\d+) segments", err).group(1))
    if window == ("--bam-window-kb", "1") and case == "all":
        assert segs(err1) == sum(1 for t in sel if N_READS[t])      # every target is larger than the window: one per segment, the empty one rides along
    if window == ("--bam-window-kb", "64") and case == "far_apart":
        assert segs(err1) == 1                           # distant targets coalesce into one segment
    if window == () and case == "all":
        assert segs(err1) == 1


def test_index_named_x_bai_is_used(floria_hip, data, tmp_path):
    prefix = copy_set(data, tmp_path, "x", open(data["ix"] + ".bam.bai", "rb").read(), index_name=str(tmp_path / "x.bai"))
    want, _, _ = run(floria_hip, data["plain"], tmp_path, extra=("-G", "ctg4"))
    got, err, _ = run(floria_hip, prefix, tmp_path, extra=("-G", "ctg4"))
    assert got == want
    rep = REPORT.search(err)
    assert rep and rep.group(1) == str(tmp_path / "x.bai") and int(rep.group(3)) < int(rep.group(4))


def _index_with_begin(data, tid, new_begin):
    """the index with every chunk begin (and the pseudo-bin's ref_beg) of `tid` that equals its begin(t) replaced"""
    raw = bytearray(open(data["ix"] + ".bam.bai", "rb").read())
    old = struct.pack("<Q", data["model"]["begin"][tid])
    assert raw.count(old) >= 2
    return bytes(raw.replace(old, struct.pack("<Q", new_begin)))


def _refusals(data):
    good = open(data["ix"] + ".bam.bai", "rb").read()
    m = data["model"]
    size = os.path.getsize(data["ix"] + ".bam")
    return {
        "truncated": good[:len(good) // 2],
        "truncated_in_the_header": good[:6],
        "wrong_magic": b"CSI\1" + good[4:],
        "n_ref_off_by_one": good[:4] + struct.pack("<I", 9) + good[8:len(good) - 8] + struct.pack("<II", 0, 0) + good[len(good) - 8:],
        "begin_beyond_the_file": _index_with_begin(data, 4, (size + 1000) << 16),
        "begin_not_on_a_member": _index_with_begin(data, 4, m["begin"][4] + (3 << 16)),
        "begin_at_another_targets_record": _index_with_begin(data, 4, m["begin"][2]),
    }


@pytest.mark.parametrize("what", ["truncated", "truncated_in_the_header", "wrong_magic", "n_ref_off_by_one", "begin_beyond_the_file", "begin_not_on_a_member",
                                  "begin_at_another_targets_record"])
def test_a_bad_index_is_refused_by_name(floria_hip, data, tmp_path, what):
    prefix = copy_set(data, tmp_path, "bad", _refusals(data)[what])
    _, err, rc = run(floria_hip, prefix, tmp_path, ok=False)
    assert rc != 0
    assert "floria-hip: error:" in err and prefix + ".bam.bai" in err, err
    assert not os.path.exists(tmp_path / "out")
    # and --no-index reads the same file as if the index were not there
    got, _, _ = run(floria_hip, prefix, tmp_path, extra=("--no-index",))
    want, _, _ = run(floria_hip, data["plain"], tmp_path)
    assert got == want


def test_an_index_older_than_the_bam_warns_and_is_used(floria_hip, data, tmp_path):
    prefix = copy_set(data, tmp_path, "old", open(data["ix"] + ".bam.bai", "rb").read())
    st = os.stat(prefix + ".bam")
    os.utime(prefix + ".bam.bai", ns=(st.st_atime_ns, st.st_mtime_ns - 5_000_000_000))
    want, err0, _ = run(floria_hip, data["plain"], tmp_path, extra=("-G", "ctg2", "ctg6", "ctg7"))
    got, err1, _ = run(floria_hip, prefix, tmp_path, extra=("-G", "ctg2", "ctg6", "ctg7"))
    assert got == want
    assert "is older than" not in err0
    assert sum(1 for ln in err1.splitlines() if "warning: the index" in ln and "is older than" in ln) == 1
    assert REPORT.search(err1)
    # a fresh index does not warn
    os.utime(prefix + ".bam.bai", ns=(st.st_atime_ns, st.st_mtime_ns + 5_000_000_000))
    _, err2, _ = run(floria_hip, prefix, tmp_path, extra=("-G", "ctg2"))
    assert "is older than" not in err2


def test_unindexed_stderr_and_peak_are_those_of_no_index(floria_hip, data, tmp_path):
    seconds = re.compile(r"\d+\.\d+s")
    for extra in ((), ("--bam-window-kb", "8"), ("-G", "ctg7", "--bam-window-kb", "8")):
        a, err_a, _ = run(floria_hip, data["plain"], tmp_path, extra=extra)
        b, err_b, _ = run(floria_hip, data["ix"], tmp_path, extra=("--no-index", *extra))
        assert a == b
        norm = lambda e, p: seconds.sub("<s>", e.replace(p, "SET"))
        assert norm(err_a, data["plain"]) == norm(err_b, data["ix"])
        peak = lambda e: re.search(r"largest inflated buffer (\d+) MiB", e).group(1)
        assert peak(err_a) == peak(err_b)
        assert "BAM index" not in err_a


def test_estimate_pass_reads_from_the_start_whatever_the_selection(floria_hip, data, tmp_path):
    # without -e / -l the estimate samples the file from its first record on, indexed or not: the same estimate, then the same Frags
    def go(prefix, extra):
        dump = str(tmp_path / "est.txt")
        r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "out"), "--ingest-only", "--pileup", "host",
                            "--dump-frags", dump, "--snp-count-filter", "20", "-t", "2", "-G", "ctg7", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return open(dump).read(), [ln for ln in r.stderr.splitlines() if ln.startswith("Estimated")]
    a, b = go(data["ix"], ()), go(data["ix"], ("--no-index",))
    assert a == b and len(a[1]) == 1


def test_usage_names_the_index(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert "--no-index" in r.stderr and ".bam.bai" in r.stderr


def test_stream_and_index_reader_under_address_and_ub_sanitizers(data, tmp_path):
    """BamStream, the .bai reader and the record decode in a stand-alone host program (floria_amd/host/bam_index_check.cpp, its own main, no device library) built
    with -fsanitize=address,undefined: once over the set with and without the index, and over every malformed index.  Exit 0 or 3 (refused by the library);
    a sanitizer report ends the program with another status."""
    subprocess.check_call(["make", "-C", HOST, "bam-index-check-asan"], stdout=subprocess.DEVNULL, timeout=900)
    exe = os.path.join(HOST, "bam-index-check-asan")

    def check(prefix, args, want_rc):
        r = subprocess.run([exe, prefix + ".bam", *args], capture_output=True, text=True, timeout=120)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert r.returncode == want_rc, (args, r.returncode, r.stdout, r.stderr)
        return r.stdout

    targets = lambda out: {int(ln.split()[1][:-1]): ln for ln in out.splitlines() if ln.startswith("target ")}
    whole = targets(check(data["plain"], ["--window", "4096", "--threads", "3"], 0))
    assert sorted(whole) == [t for t in range(8) if N_READS[t]]
    assert all(f": {N_READS[t]} records" in whole[t] for t in whole)
    for tids in (["0"], ["7"], ["3"], ["1", "2"], ["0", "7"], [str(t) for t in range(8)]):
        for window in ("1", "1000000"):          # the same records, field for field, as the unindexed stream gives for these targets
            got = targets(check(data["ix"], ["--select", *tids, "--window", window], 0))
            assert got == {int(t): whole[int(t)] for t in tids if N_READS[int(t)]}
    check(data["ix"], ["--window", "4096"], 0)                   # an index and no selection: the stream from the start
    for what, index_bytes in _refusals(data).items():
        prefix = copy_set(data, tmp_path, "san_" + what, index_bytes)
        out = check(prefix, ["--select", "2", "4", "7", "--window", "1"], 3)
        assert "refused:" in out and prefix + ".bam.bai" in out, (what, out)
