"""`-m gpu`: floria-hip --pileup resident against --pileup host on the same inputs: the same files byte for byte, and the same resident arrays behind every contig's
handle (--dump-handles: floria_hip_contig_download fields 0-6, field 7 where both routes carry a set order) - at -e 0.03125, where both arithmetics are one function,
and at -e 0.04, where the run phases in the reference's running sums on set orders (replayed on the host in one route, derived on the device in the other).
Also the two arrays floria_hip_drop_monomorphic returns for a host that keeps headers only."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from floria_amd.pileup import Pileup
from tests import mono_model as mm
from tests import plan_model as plm
from tests.test_gpu_pileup import hand_built, run_route

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
EPS = (0.03125, 0.04)


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def run_resident(floria_hip, prefix, out, eps, extra, route="resident"):
    """run_route of tests/test_gpu_pileup.py without --dump-frags (refused under --pileup resident)"""
    if os.path.exists(out):
        shutil.rmtree(out)
    cmd = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", out, "-e", repr(eps), "-l", "10000", "-t", "4", "--pileup", route, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    tree = {}
    for dp, _, fs in os.walk(out):
        for f in fs:
            if f != "cmd.log":
                tree[os.path.relpath(os.path.join(dp, f), out)] = open(os.path.join(dp, f), "rb").read()
    return tree, r.stderr


def parse_handles(path):
    """--dump-handles -> [(contig, ids, {field: the line's numbers as text})] in file order"""
    out = []
    for line in open(path):
        t = line.rstrip("\n").split("\t", 2)
        if t[0] == "#CONTIG":
            out.append((t[1], None, {}))
        elif t[0] == "#IDS":
            out[-1] = (out[-1][0], t[1:], out[-1][2])
        elif t[0] == "#FIELD":
            out[-1][2][int(t[1])] = t[2] if len(t) > 2 else ""
    return out


def routes_agree(floria_hip, tmp_path, prefix, extra=(), eps_list=EPS, seq_pos=False, min_files=4):
    """host and resident write to the SAME output directory one after the other (its path is part of every vartig header) -> [(host stderr, resident stderr)]"""
    errs = []
    for eps in eps_list:
        out, dump = str(tmp_path / "out"), str(tmp_path / "frags.txt")
        hh, rh, hs, rs = (str(tmp_path / n) for n in ("handles_host.txt", "handles_resident.txt", "seqpos_host.txt", "seqpos_resident.txt"))
        sp = lambda f: ("--dump-seq-pos", f) if seq_pos else ()
        host_tree, _, host_err = run_route(floria_hip, prefix, out, dump, "host", eps, (*extra, "--dump-handles", hh, *sp(hs)))
        res_tree, res_err = run_resident(floria_hip, prefix, out, eps, (*extra, "--dump-handles", rh, *sp(rs)))
        assert "Pileup on the device:" in res_err and "Resident contigs:" in res_err and "no cell" in res_err
        assert sorted(res_tree) == sorted(host_tree) and len(host_tree) >= min_files, (sorted(res_tree), sorted(host_tree))
        for fn in host_tree:
            assert res_tree[fn] == host_tree[fn], f"{fn} differs at -e {eps}"
        a, b = parse_handles(hh), parse_handles(rh)
        assert [(c, ids) for c, ids, _ in a] == [(c, ids) for c, ids, _ in b], f"contigs or read ids of the handles differ at -e {eps}"
        for (c, _, fa), (_, _, fb) in zip(a, b):
            for k in range(7):
                assert fa[k] == fb[k], f"field {k} of contig {c} differs at -e {eps}"
            if 7 in fa and 7 in fb:
                assert fa[7] == fb[7], f"set order of contig {c} differs at -e {eps}"
        if seq_pos:
            assert open(hs).read() == open(rs).read() and os.path.getsize(hs) > 1000, f"--dump-seq-pos differs at -e {eps}"
        errs.append((host_err, res_err))
    return errs


def filter_counts(err):
    m = re.search(r"(\d+) SNPs removed, (\d+) reads dropped", err)
    return int(m.group(1)), int(m.group(2))


def assert_filter_was_exercised(errs):
    for _, res_err in errs:
        snps, reads = filter_counts(res_err)
        assert snps >= 1 and reads >= 1, (snps, reads)


# ---- the data sets ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy(tmp_path_factory, floria_hip):
    c = synth.make_config_contig(1, 1, 0.6, keep_layout=True)
    prefix = str(tmp_path_factory.mktemp("noisy") / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12)
    plm.add_read_on_a_monomorphic_snp(floria_hip, prefix)             # (the set as generated loses SNPs to --ignore-monomorphic, but no read)
    return prefix


@pytest.fixture(scope="module")
def paired(tmp_path_factory):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path_factory.mktemp("paired") / "d")
    synth_bam.write_dataset(prefix, [c], seed=7)
    plm.add_case_records(prefix)
    return prefix


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("hand") / "h")
    hand_built(prefix)
    plm.add_case_records(prefix)
    return prefix


@pytest.fixture(scope="module")
def edited(tmp_path_factory, floria_hip):
    c = synth.make_config_contig(1, 0, 0.5, keep_layout=True)
    prefix = str(tmp_path_factory.mktemp("edited") / "l")
    synth_bam.write_dataset(prefix, [c], seed=7, edit_frac=0.5)
    plm.add_read_on_a_monomorphic_snp(floria_hip, prefix)             # (as for the noisy set)
    return prefix


HAND = ("--snp-count-filter", "10", "--supp-aln-dist-cutoff", "10000")


def realign_line(err):
    return re.search(r"Realignment: \d+ calls scored on the device behind the walk \([^)]*\)", err).group(0)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------
def test_noisy_long_reads_realigned_behind_the_walk(floria_hip, tmp_path, noisy):
    errs = routes_agree(floria_hip, tmp_path, noisy)
    _, fused_err = run_resident(floria_hip, noisy, str(tmp_path / "out"), EPS[0], (), route="fused")
    for _, res_err in errs:
        assert realign_line(res_err) == realign_line(fused_err)
        assert int(re.search(r"Realignment: (\d+) calls scored on the device behind", res_err).group(1)) > 1000


def test_noisy_long_reads_with_a_block_walk(floria_hip, tmp_path, noisy):
    errs = routes_agree(floria_hip, tmp_path, noisy, extra=("--realign", "block:8,max,right"))
    assert all("fixed-block walk block:8,max,right" in res_err for _, res_err in errs)


def test_noisy_long_reads_without_realignment(floria_hip, tmp_path, noisy):
    errs = routes_agree(floria_hip, tmp_path, noisy, extra=("--no-realign",))
    assert all("behind the walk" not in res_err for _, res_err in errs)


def test_paired_short_reads_on_derived_set_orders(floria_hip, tmp_path, paired):
    errs = routes_agree(floria_hip, tmp_path, paired, extra=("-l", "500"))
    host_err, res_err = errs[1]                                                   # -e 0.04: the reference arithmetic
    assert "replayed on the host" in host_err
    m = re.search(r"Arithmetic: the set orders of (\d+) fragments merged from several alignments were derived on the device", res_err)
    assert m and int(m.group(1)) > 50
    assert "derived on the device" not in errs[0][1]


def test_hand_built_supplementary_and_paired_set_with_output_reads(floria_hip, tmp_path, hand):
    routes_agree(floria_hip, tmp_path, hand, extra=(*HAND, "--output-reads"), seq_pos=True)
    lines = {l.split("\t")[0]: l.rstrip("\n").split("\t")[1:] for l in open(tmp_path / "seqpos_resident.txt") if not l.startswith("#")}
    mates = lambda name: {int(x.split(":")[1]) for x in lines[name]}
    # (SNPs are 500 bases apart here: the mates of a pair share their one SNP, and the shared SNP takes the word of the part merged last - the second mate's)
    assert mates("x_pair_shared") == {1} and mates("x_pair_128_first") == {1} and mates("x_pair_no_cell_mate") == {1} and mates("supp_near") == {0}
    assert len(lines["x_pair_shared"]) == 1 and len(lines["supp_near"]) >= 4
    assert max(int(x.split(":")[2]) for x in lines["supp_near"]) >= 1200          # the supplementary piece's positions, shifted by its hard clip


def test_edited_cigars_with_output_reads_and_extra_trimming(floria_hip, tmp_path, edited):
    routes_agree(floria_hip, tmp_path, edited, extra=("--output-reads", "--extra-trimming"), seq_pos=True)


@pytest.mark.parametrize("which", ["noisy", "paired", "hand", "edited"])
def test_ignore_monomorphic(floria_hip, tmp_path, request, which):
    prefix = request.getfixturevalue(which)
    extra = {"noisy": (), "paired": ("-l", "500"), "hand": HAND, "edited": ()}[which]
    assert_filter_was_exercised(routes_agree(floria_hip, tmp_path, prefix, extra=(*extra, "--ignore-monomorphic")))


def test_ignore_monomorphic_with_output_reads_on_set_orders(floria_hip, tmp_path, paired):
    errs = routes_agree(floria_hip, tmp_path, paired, extra=("-l", "500", "--ignore-monomorphic", "--output-reads"), eps_list=(0.04,), seq_pos=True)
    assert_filter_was_exercised(errs)
    assert "derived on the device" in errs[0][1]


@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """eight small long-read contigs and one of paired short reads (the sizes of tests/test_gpu_pileup.py's nine halved: the suite runs every one of these eight times)"""
    cs = [synth.make_config_contig(4, 20 + i, 0.12 + 0.02 * i, keep_layout=True) for i in range(8)] + [synth.make_config_contig(3, 5, 0.1, keep_layout=True)]
    prefix = str(tmp_path_factory.mktemp("nine") / "d")
    synth_bam.write_dataset(prefix, cs, seed=7, edit_frac=0.5)
    return prefix


NINE = ("--snp-count-filter", "50")


def test_nine_contigs_in_batches_of_three(floria_hip, tmp_path, nine):
    for _, res_err in routes_agree(floria_hip, tmp_path, nine, extra=(*NINE, "--batch-contigs", "3"), min_files=30):
        assert "Batches 3;" in res_err and "Resident contigs: 9 assembled" in res_err


def test_nine_contigs_of_five_rounds_in_one_batch(floria_hip, tmp_path, nine):
    """-t 1: two contigs per ingest round, so handles made by five pileup + assemble calls meet in one batch, and the residency is renewed between the rounds"""
    for _, res_err in routes_agree(floria_hip, tmp_path, nine, extra=(*NINE, "-t", "1"), min_files=30):
        assert "Batches 1;" in res_err and int(re.search(r"Pileup on the device: \d+ records, \d+ blob bytes in (\d+) calls", res_err).group(1)) == 5


def test_nine_contigs_in_several_bam_segments(floria_hip, tmp_path, nine):
    for _, res_err in routes_agree(floria_hip, tmp_path, nine, extra=(*NINE, "--bam-window-kb", "64", "-t", "1"), min_files=30):
        assert int(re.search(r"BAM: \d+ records in (\d+) segments", res_err).group(1)) > 1
        assert int(re.search(r"Pileup on the device: \d+ records, \d+ blob bytes in (\d+) calls", res_err).group(1)) > 1


def merged_dataset(prefix, parts):
    """the one-contig data sets `parts` (prefixes) as one data set of several contigs, in that order"""
    targets, rows = [], []
    with open(prefix + ".fa", "w") as fa, open(prefix + ".vcf", "w") as vcf:
        vcf.write("##fileformat=VCFv4.2\n")
        body = []
        for tid, p in enumerate(parts):
            t, recs = plm.read_bam(p + ".bam")
            assert len(t) == 1
            targets.append(t[0])
            vcf.write(f"##contig=<ID={t[0][0]},length={t[0][1]}>\n")
            body += [l for l in open(p + ".vcf") if not l.startswith("#")]
            fa.write(open(p + ".fa").read())
            rows += [r["raw"][:4] + np.int32(tid).tobytes() + r["raw"][8:] for r in recs]
        vcf.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n" + "".join(body))
    synth_bam.write_bam(prefix + ".bam", targets, rows)


def test_contig_with_a_five_allele_site_keeps_the_host_walk_in_a_mixed_batch(floria_hip, tmp_path, edited):
    five = str(tmp_path / "five")
    hand_built(five, five_alleles=True)
    prefix = str(tmp_path / "m")
    merged_dataset(prefix, [edited, five])
    for _, res_err in routes_agree(floria_hip, tmp_path, prefix, extra=(*HAND, "--no-realign", "--output-reads"), min_files=8):
        assert res_err.count("keeps the host walk") == 1 and "contig c " in res_err
        assert "Resident contigs: 1 assembled" in res_err


def test_contig_without_passing_records_and_contig_of_snpless_fragments(floria_hip, tmp_path, edited):
    """three contigs: one that phases; `quiet`, whose only records fail the MAPQ cutoff; `bare`, whose every read lies between two SNPs.  Neither of the two gets a directory."""
    rng = np.random.default_rng(11)
    for name, mapq, at in (("quiet", 3, 1000), ("bare", 60, 5020)):
        p = str(tmp_path / name)
        ref = synth_bam.BASES[rng.integers(0, 4, size=20000)]
        snps = [1000 + 100 * i for i in range(40)] + [9000 + 100 * i for i in range(40)]                 # nothing between 4 900 and 9 000
        with open(p + ".fa", "w") as f:
            f.write(f">{name}\n" + bytes(ref).decode() + "\n")
        with open(p + ".vcf", "w") as f:
            for q in snps:
                f.write(f"{name}\t{q + 1}\t.\t{chr(ref[q])}\t{'ACGT'[('ACGT'.index(chr(ref[q])) + 1) % 4]}\t50\tPASS\t.\tGT\t0/1\n")
        recs = [synth_bam.bam_record(0, at + 30 * k, f"{name}{k}", 0, mapq, [("M", 900)], bytes(ref[at + 30 * k:at + 30 * k + 900]), np.full(900, 30, np.uint8)) for k in range(20)]
        synth_bam.write_bam(p + ".bam", [(name, 20000)], recs)
    prefix = str(tmp_path / "m")
    merged_dataset(prefix, [str(tmp_path / "quiet"), edited, str(tmp_path / "bare")])
    for host_err, res_err in routes_agree(floria_hip, tmp_path, prefix, extra=("--snp-count-filter", "10")):
        for err in (host_err, res_err):
            assert "Number of reads passing filtering: 0 (quiet)" in err and "Number of reads passing filtering: 0 (bare)" in err
        assert not os.path.exists(tmp_path / "out" / "quiet") and not os.path.exists(tmp_path / "out" / "bare")


def test_ingest_only_plans_from_the_summary_as_the_host_walk_plans_from_its_frags(floria_hip, tmp_path, hand, paired):
    """--ingest-only --pileup resident walks, plans and assembles and stops; its --dump-plan, made from the device's per-record spans, is the host route's"""
    for prefix, extra in ((hand, HAND), (paired, ())):
        plans = {}
        for route in ("host", "resident"):
            plan = str(tmp_path / f"plan_{route}.txt")
            r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.04", "-l", "10000", "-t", "4",
                                "--ingest-only", "--pileup", route, "--dump-plan", plan, *extra], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            plans[route] = open(plan).read()
            assert ("Resident contigs: 1 assembled" in r.stderr) == (route == "resident") and not os.path.exists(tmp_path / "unused")
        assert plans["host"] == plans["resident"] and plans["host"].count("\nF\t") > 200 and "\nS\t" in plans["host"]


# ---- the new fields of floria_mono_result---------------------------------------------------------------------------------------------------------------
def test_mono_result_returns_the_survivors_first_and_last_snp(gpu_ctx, hip_lib):
    from tests.test_gpu_mono import random_contig, take
    from tests.test_gpu_assemble import free_all
    rng = np.random.default_rng(77)
    big = random_contig(rng, 150, 320, lengths=(1, 65, 290))                                  # reads of 1, 65 and 290 cells: more than one trip of the filter's loops
    gone = Pileup.from_reads([(np.arange(s, s + 5), np.zeros(5, np.uint8), np.full(5, 30)) for s in range(1, 21)])      # one allele everywhere: loses every read
    mid = random_contig(rng, 90, 60)
    pileups, counts, eps = [big, gone, mid], [320, 24, 60], 0.03125
    assert sorted(np.diff(big.read_off).tolist())[-2:] == [65, 290] and 1 in np.diff(big.read_off).tolist()
    want, want_res = mm.drop_batch(pileups, counts, eps)
    want_first = np.concatenate([p.first for p in want]).astype(np.uint32)
    want_last = np.concatenate([p.last for p in want]).astype(np.uint32)
    assert want[1].n_reads == 0 and want[0].n_reads > 100
    old = want_res["old_read"][:want[0].n_reads].astype(np.int64)
    assert (want[0].first != big.first[old]).any() and (want[0].last != big.last[old]).any()          # ends that moved: a copy of the old ones would not pass
    src = gpu_ctx.upload_batch(pileups)
    batch, res = gpu_ctx.drop_monomorphic(src, counts, eps)
    got = take(hip_lib, gpu_ctx, batch, res)
    try:
        assert np.array_equal(res["old_read"], want_res["old_read"]) and np.array_equal(res["read_off"], want_res["read_off"])
        assert res["new_first"].dtype == np.uint32 and np.array_equal(res["new_first"], want_first)
        assert res["new_last"].dtype == np.uint32 and np.array_equal(res["new_last"], want_last)
        for g, w in zip(got, want):                                                           # ... and they are what the output handles hold
            assert np.array_equal(g.download("first", w.n_reads), w.first) and np.array_equal(g.download("last", w.n_reads), w.last)
    finally:
        free_all(got, src)
