"""`-m "not gpu"`: the host side of floria-hip --pileup resident that needs no device.  The fragment plan (--dump-plan, made from headers alone) equals the model of
tests/plan_model.py, and plan o assemble - tests/assemble_model.py applied to the dumped plan and to the per-record cells of tests/pileup_model.py - reproduces the
Frags of the host route (--dump-frags) exactly: the proof, without a GPU, that what the resident route asks the device to assemble is what the host route builds.
The runs pass --no-realign: the model's cells are the walk's, and realignment changes alleles only, which no decision of the plan reads.  Also the driver's refusals and
the ctypes mirror of the extended floria_mono_result."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import assemble_model as am
from tests import pileup_model as pm
from tests import plan_model as plm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def check_set(floria_hip, prefix, tmp_path, cutoff, extra=()):
    """-> (dumped plan of the contig, records, walked cells): the plan equals the model's, plan o assemble equals --dump-frags, and every case is there"""
    from tests.test_gpu_cli import parse_frag_dump
    plan_file, frag_file = prefix + ".plan", prefix + ".frags"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.03", "-l", "10000",
                        "--ingest-only", "--no-realign", "--pileup", "host", "--supp-aln-dist-cutoff", str(cutoff), "--dump-plan", plan_file, "--dump-frags", frag_file, *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    targets, records = plm.read_bam(prefix + ".bam")
    assert len(targets) == 1
    name = targets[0][0]
    table = pm.read_vcf_tables(prefix + ".vcf", [name])[name]
    model = plm.plan_contig(records, table, cutoff)
    dumped = plm.parse_plan(plan_file)[name]
    assert len(model["frags"]) > 50
    assert plm.same_plan(model, dumped)
    # plan o assemble == the host's Frags: ids, order, first, last, every snp:allele:qual
    walked = pm.walk_records(records, [table])
    index = {(rec["name"], rec["flag"], rec["pos"]): i for i, rec in enumerate(records)}
    assert len(index) == len(records)
    host = parse_frag_dump(frag_file)[name]
    assert [g["name"] for g in host["reads"]] == [f["name"] for f in dumped["frags"]]
    for g, f in zip(host["reads"], dumped["frags"]):
        snp, allele, qual = am.merge_fragment(walked, [index[p[:3]] for p in f["parts"]])
        assert g["cells"] == list(zip(snp.tolist(), allele.tolist(), qual.tolist())), g["name"]
        assert (g["first"], g["last"]) == (f["first"], f["last"]) == (int(snp[0]), int(snp[-1])), g["name"]
    assert [s[0] for s in host["snpless"]] == [f["name"] for f in dumped["snpless"]]
    # the cases, counted in the dumped plan
    cells_of = lambda p: set(am.record_cells(walked, index[p[:3]])[0].tolist())
    pairs = [f for f in dumped["frags"] + dumped["snpless"] if len(f["parts"]) == 2 and f["parts"][1][3] == 1]
    assert sum(1 for f in pairs if cells_of(f["parts"][0]) & cells_of(f["parts"][1])) >= 1, "no pair whose mates share a SNP"
    assert sum(1 for f in pairs if f["parts"][1][1] & 128 and not f["parts"][1][1] & 64 and f["parts"][1][1] < f["parts"][0][1]) >= 1, "no pair in which flag 128 sorts first"
    assert sum(1 for f in pairs if not cells_of(f["parts"][0]) and cells_of(f["parts"][1])) >= 1, "no pair whose base has no cell"
    by_name = {}
    for rec in records:
        if plm.passes(rec["flag"], rec["mapq"]):
            by_name.setdefault(rec["name"], []).append(rec["flag"])
    supp_only = [n for n, fl in by_name.items() if all(x & 2048 for x in fl)]
    planned = {f["name"] for f in dumped["frags"] + dumped["snpless"]}
    assert supp_only and not planned & set(supp_only), "no group of supplementary records only"
    assert len(dumped["snpless"]) >= 1, "no fragment without cells"
    assert all(all(m == 0 for _, _, _, m in f["parts"]) for f in dumped["frags"] + dumped["snpless"] if f not in pairs)
    return dumped, records, walked


def primary_only_groups(dumped, records):
    """names with a supplementary record that passes, planned as one part"""
    with_supp = {rec["name"] for rec in records if rec["flag"] & 2048 and plm.passes(rec["flag"], rec["mapq"])}
    return sorted(f["name"] for f in dumped["frags"] + dumped["snpless"] if f["name"] in with_supp and len(f["parts"]) == 1)


def test_plan_of_the_hand_built_supplementary_set_at_two_cutoffs(floria_hip, tmp_path):
    from tests.test_gpu_pileup import hand_built
    prefix = str(tmp_path / "h")
    hand_built(prefix)
    plm.add_case_records(prefix)
    near, records, _ = check_set(floria_hip, prefix, tmp_path, 10000, extra=("--snp-count-filter", "10"))
    merged = {f["name"]: len(f["parts"]) for f in near["frags"]}
    assert merged["supp_near"] == 2 and merged["supp_far"] == 1 and merged["x_supp_merge"] == 2
    assert primary_only_groups(near, records) == ["supp_far"]
    # a cutoff below the 4 000 bases between supp_near's pieces: that group keeps its primary only as well
    tight, records, _ = check_set(floria_hip, prefix, tmp_path, 1000, extra=("--snp-count-filter", "10"))
    assert {"supp_far", "supp_near"} <= set(primary_only_groups(tight, records))


def test_plan_of_paired_short_reads(floria_hip, tmp_path):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path / "p")
    synth_bam.write_dataset(prefix, [c], seed=7)
    plm.add_case_records(prefix)
    dumped, _, _ = check_set(floria_hip, prefix, tmp_path, 40000)
    assert sum(1 for f in dumped["frags"] if len(f["parts"]) == 2) > 50


def test_plan_of_long_reads_with_edited_cigars(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 0, 0.5, keep_layout=True)
    prefix = str(tmp_path / "l")
    synth_bam.write_dataset(prefix, [c], seed=7, edit_frac=0.5)
    plm.add_case_records(prefix)
    _, records, _ = check_set(floria_hip, prefix, tmp_path, 40000)
    assert sum(1 for rec in records if len(rec["cigar"]) > 1) > 20


def test_the_plan_model_on_a_group_it_can_be_checked_by_hand():
    """three SNPs 1000 bases apart; a pair with flags 129 / 145, a supplementary-only name, a primary with a far supplementary piece at cutoff 500 and at 5000"""
    table = pm.SnpTable([1000, 2000, 3000], [[65, 67, 0, 0]] * 3, [2, 2, 2])
    rec = lambda name, pos, flag, n=20: dict(name=name, pos=pos, flag=flag, mapq=60, cigar=[("M", n)], seq=b"A" * n, qual=np.full(n, 30, np.uint8), contig=0)
    records = [rec("p", 990, 129), rec("s", 990, 2048), rec("q", 995, 0), rec("p", 1990, 145), rec("q", 2990, 2048), rec("e", 1500, 0), rec("low", 990, 0) | dict(mapq=3)]
    plan = plm.plan_contig(records, table, 500)
    assert [(f["name"], f["first"], f["last"], f["parts"]) for f in plan["frags"]] == [
        ("p", 1, 2, [("p", 145, 1990, 0), ("p", 129, 990, 1)]), ("q", 1, 1, [("q", 0, 995, 0)])]
    assert [f["name"] for f in plan["snpless"]] == ["e"]
    plan = plm.plan_contig(records, table, 5000)
    assert [(f["name"], f["first"], f["last"], f["parts"]) for f in plan["frags"]] == [
        ("q", 1, 3, [("q", 0, 995, 0), ("q", 2048, 2990, 0)]), ("p", 1, 2, [("p", 145, 1990, 0), ("p", 129, 990, 1)])]


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------------
def test_usage_names_the_resident_route(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pileup host|device|fused" in r.stderr and "--pileup host|device|fused|resident" in r.stderr
    r = subprocess.run([floria_hip, "-b", "x.bam", "-v", "x.vcf", "-r", "x.fa", "--pileup", "fusion"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pileup takes host or device" in r.stderr and "fused" in r.stderr and "resident" in r.stderr


def test_resident_with_several_devices_is_refused_before_anything_is_read(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "-b", str(tmp_path / "none.bam"), "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--pileup", "resident", "--devices", "0,1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pileup resident runs on one device" in r.stderr and "the context that walked" in r.stderr and "precede the walk" in r.stderr
    assert "none.bam" not in r.stderr and not os.path.exists(tmp_path / "o")


def test_resident_with_dump_frags_is_refused_before_anything_is_read(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "-b", str(tmp_path / "none.bam"), "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--pileup", "resident", "--dump-frags",
                        str(tmp_path / "f.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dump-frags is not available under --pileup resident" in r.stderr and "folded into weights on the device" in r.stderr
    assert "none.bam" not in r.stderr and not os.path.exists(tmp_path / "o") and not os.path.exists(tmp_path / "f.txt")


def test_dump_plan_needs_ingest_only(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "-b", str(tmp_path / "none.bam"), "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--dump-plan", str(tmp_path / "p.txt")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dump-plan needs --ingest-only" in r.stderr


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------------------
def test_mono_result_mirror_matches_the_header_layout(tmp_path):
    """sizeof / offsetof of floria_mono_result, measured by gcc, equal the mirror in floria_amd/_capi.py; the two new arrays stand at its end"""
    from floria_amd import _capi as capi
    cls = capi.CMonoResult
    fields = [f for f, _ in cls._fields_]
    assert fields[-2:] == ["new_first", "new_last"] and fields[:7] == ["n_contigs", "read_off", "old_read", "removed", "n_removed_snps", "n_removed_cells", "n_dropped_reads"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "floria_hip.h"', "int main(void) {", '  printf("%zu", sizeof(floria_mono_result));']
    lines += [f'  printf(" %zu", offsetof(floria_mono_result, {f}));' for f in fields]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    size, *offs = subprocess.check_output([str(tmp_path / "layout")], text=True).split()
    assert int(size) == C.sizeof(cls)
    assert [int(o) for o in offs] == [getattr(cls, f).offset for f in fields]
