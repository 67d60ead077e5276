"""`-m "not gpu"`: the yardstick of the fused device realignment (tests/pileup_realign_model.py) is pinned to the product's host route, the shared test inputs
hold every boundary of the rule and can tell wrong rules from the right one, the new ctypes mirrors match the header, and the driver knows --pileup fused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import pileup_model as pm
from tests import pileup_realign_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def host_route(floria_hip, prefix, tmp_path, extra=()):
    """the fragments of floria-hip --ingest-only with the realignment ON (scored on the host: no device is involved)"""
    from tests.test_gpu_cli import parse_frag_dump
    dump = prefix + ".frags"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.03", "-l", "10000",
                        "--ingest-only", "--dump-frags", dump, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return parse_frag_dump(dump)


def model_cells_by_name(records, tables, refs, member):
    """read name -> [(snp, allele, qual)] ascending by SNP, the records of a name merged the way combine_frags does (a later record's call replaces an earlier one's)"""
    (cell_off, snp, allele, qual, _sp, _re), counts, _ = rm.realign_records(records, tables, refs, member=member, use_shortcut=True)
    by_name = {}
    for i, r in enumerate(records):
        cells = by_name.setdefault(r["name"], {})
        for x in range(int(cell_off[i]), int(cell_off[i + 1])):
            cells[int(snp[x])] = (int(snp[x]), int(allele[x]), int(qual[x]))
    return {nm: [c[k] for k in sorted(c)] for nm, c in by_name.items()}, counts


@pytest.mark.parametrize("member", [None, (8, 0, 0)], ids=["exact", "block:8,max,right"])
def test_model_reproduces_the_host_route_on_noisy_long_reads(floria_hip, tmp_path, member):
    c = synth.make_config_contig(1, 1, 0.6 if member is None else 0.25, keep_layout=True)            # (the walk's model is the slower one: a smaller contig for it)
    prefix = str(tmp_path / "d")
    ex = synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12, realign=False)[c.name]
    table = pm.read_vcf_tables(prefix + ".vcf", [c.name])[c.name]
    ref = "".join(l.strip() for l in open(prefix + ".fa") if not l.startswith(">")).encode()
    records = []
    for name, alns in ex["read_alignments"].items():
        assert len(alns) == 1
        pos, seq, cig, qual = alns[0]
        records.append(dict(pos=pos, flag=0, contig=0, cigar=cig, seq=seq, qual=np.frombuffer(qual, np.uint8), name=name))
    want, counts = model_cells_by_name(records, [table], [ref], member)
    lim = 1000 if member is None else 500
    assert counts["scored"] > lim and counts["shortcut"] > lim and counts["changed"] > 0, counts
    from tests.realign_walk_model import spec
    got = host_route(floria_hip, prefix, tmp_path, extra=() if member is None else ("--realign", spec(member)))[c.name]
    assert len(got["reads"]) > (100 if member is None else 25)
    for g in got["reads"]:
        assert g["cells"] == want[g["name"]], g["name"]


def hand_built_files(prefix):
    """one contig, SNPs every 100 bases, noisy plain reads, and two primary + supplementary pairs whose supplementary piece is hard-clipped by less than its length,
    so that the shifted seq_pos of most of its calls stays inside the record and selects other bases -> (records, SnpTable, ref bytes)"""
    rng = np.random.default_rng(11)
    clen = 8000
    ref = synth_bam.BASES[rng.integers(0, 4, size=clen)].copy()
    snp_pos = 500 + 100 * np.arange(70)
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    alt = np.array([nxt[int(ref[q])] for q in snp_pos], np.uint8)
    with open(prefix + ".fa", "w") as f:
        f.write(">c\n" + bytes(ref).decode() + "\n")
    with open(prefix + ".vcf", "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=c,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n" % clen)
        for i, q in enumerate(snp_pos):
            f.write(f"c\t{q + 1}\t.\t{chr(ref[q])}\t{chr(alt[i])}\t50\tPASS\t.\tGT\t0/1\n")
    recs = []

    def add(name, pos, flag, cigar, noise):
        n = sum(ln for op, ln in cigar if op in pm.Q_OPS)
        lead = sum(ln for op, ln in cigar[:1] if op == "S")
        s = ref[pos - lead:pos - lead + n].copy()
        for i, q in enumerate(snp_pos):
            if pos - lead <= q < pos - lead + n and (i + len(recs)) % 3:
                s[q - pos + lead] = alt[i]
        hit = rng.random(n) < noise
        s[hit] = synth_bam.BASES[rng.integers(0, 4, size=int(hit.sum()))]
        recs.append(pm.make_record(pos, cigar, bytes(s), rng.integers(10, 40, size=n).astype(np.uint8), flag=flag, contig=0, name=name))
    for k in range(40):
        add(f"plain{k}", int(rng.integers(100, clen - 1600)), 0, [("M", 1500)], 0.1)
    add("sa", 1000, 0, [("M", 800), ("S", 400)], 0.05)
    add("sa", 2200, 2048, [("H", 40), ("M", 700)], 0.05)
    add("sb", 4000, 0, [("S", 20), ("M", 600)], 0.05)
    add("sb", 5020, 2048, [("H", 16), ("M", 410), ("H", 9)], 0.0)
    recs.sort(key=lambda r: r["pos"])
    synth_bam.write_bam(prefix + ".bam", [("c", clen)], [r["raw"] for r in recs])
    al = np.zeros((len(snp_pos), 4), np.uint8); al[:, 0] = ref[snp_pos]; al[:, 1] = alt
    return recs, pm.SnpTable(snp_pos, al, np.full(len(snp_pos), 2, np.uint8)), bytes(ref)


@pytest.mark.parametrize("member", [None, (8, 0, 0)], ids=["exact", "block:8,max,right"])
def test_model_reproduces_the_host_route_on_a_hand_built_bam_with_hard_clipped_supplementary_records(floria_hip, tmp_path, member):
    prefix = str(tmp_path / "h")
    records, table, ref = hand_built_files(prefix)
    want, counts = model_cells_by_name(records, [table], [ref], member)
    _, _, d = rm.realign_records(records, [table], [ref], use_shortcut=True)
    supp = np.isin(d["record"], [i for i, r in enumerate(records) if r["flag"] & 0x800])
    assert (supp & d["in_bounds"] & (d["q16"] != d["walked_base"])).sum() >= 3 and (supp & ~d["in_bounds"]).sum() >= 1 and counts["changed"] >= 3
    from tests.realign_walk_model import spec
    got = host_route(floria_hip, prefix, tmp_path, extra=("--snp-count-filter", "10", "--supp-aln-dist-cutoff", "100000") + (() if member is None else ("--realign", spec(member))))["c"]
    assert {g["name"] for g in got["reads"]} == set(want) and len(want) == 42
    for g in got["reads"]:
        assert g["cells"] == want[g["name"]], g["name"]


# ---- the fixtures of the GPU tests, checked with the model alone -------------------------------------------------------------------------------------
def test_crafted_case_holds_every_boundary_of_the_rule():
    recs, tables, refs, walked, (res, counts, d) = rm.cached("crafted")
    inb = d["in_bounds"]
    for v in (15, 16):
        assert (d["p"] == v).any() and (d["G"] == v).any(), v
    for back in (17, 16):
        assert (d["p"] == d["L"] - back).any() and ((d["G"] == d["R"] - back) & (d["R"] > 0)).any(), back
    # the boundary cells are on the side of the bound the rule says
    assert not inb[d["p"] == 15].any() and inb[(d["p"] == 16) & (d["G"] >= 16) & (d["G"] + 16 < d["R"]) & (d["p"] + 16 < d["L"])].all()
    assert not inb[d["p"] == d["L"] - 16].any() and inb[(d["p"] == d["L"] - 17) & (d["p"] >= 16) & (d["G"] >= 16) & (d["G"] + 16 < d["R"])].any()
    assert not inb[d["G"] == 15].any() and not inb[d["G"] == d["R"] - 16].any() and inb[d["G"] == 16].any() and inb[d["G"] == d["R"] - 17].any()
    for h in (0, 1, 2, 3):
        assert (inb & (d["h"] == h) & d["has"]).any() and (inb & (d["h"] == h) & ~d["has"]).any(), h
    assert (inb & d["non_acgt"]).any() and (inb & d["lower_ref"]).any()
    assert {int(x) for x in d["n_alleles"][inb]} == {1, 2, 3, 4}
    assert {int(x) for x in d["p"][inb] % 2} == {0, 1}
    packed = pm.pack_records(recs, pad=lambda i: i % 4)
    assert {int(x) for x in packed["seq_off"][d["record"][inb]] % 2} == {0, 1}
    off, _ = rm.pack_refs(refs)
    assert {int(x) % 2 for x in off[:2]} == {0, 1} and off[2] == off[3] and len(refs) == 3                      # (the third contig has no reference)
    supp = np.asarray([bool(r["flag"] & 0x800) and r["cigar"][0][0] == "H" for r in recs])[d["record"]]
    assert (supp & ~inb & (d["p"] + 16 >= d["L"])).any()                                                       # a shifted p that falls out of the record
    assert (supp & inb & (d["q16"] != d["walked_base"])).any()                                                  # ... and one that selects another base
    assert (np.diff(walked[0]) == 0).any()                                                                       # a record without cells
    assert (d["R"] == 0).any()


def test_sweep_is_not_thin():
    _, _, _, _, (res, counts, d) = rm.cached("sweep")
    assert counts["scored"] >= 1000 and counts["shortcut"] >= 1000 and counts["cells"] - counts["in_bounds"] >= 200 and counts["changed"] >= 200, counts


def test_the_shortcut_is_the_scoring_rule_on_the_crafted_case():
    """the model scores every cell inside the bounds; deciding the shortcut's cells by the shortcut gives the same alleles, for the exact DP and for two walks"""
    recs, tables, refs, walked, (res, counts, d) = rm.cached("crafted")
    for member in (None, (8, 0, 0), (1, 1, 1)):
        a = rm.realign_records(recs, tables, refs, member=member, walked=walked)
        b = rm.realign_records(recs, tables, refs, member=member, walked=walked, use_shortcut=True)
        assert np.array_equal(a[0][2], b[0][2]) and a[1] == b[1], member


@pytest.mark.parametrize("wrong", [dict(lo=15), dict(lo=17), dict(hi=15), dict(hi=17), dict(unshifted=True), dict(keep_n=True), dict(last_best=True)],
                         ids=["lower bound 15", "lower bound 17", "upper bound 15", "upper bound 17", "unshifted p", "N stays N", "last best"])
def test_a_wrong_rule_shows_on_the_crafted_case(wrong):
    recs, tables, refs, walked, (res, counts, d) = rm.cached("crafted")
    other = rm.realign_records(recs, tables, refs, walked=walked, **wrong)[0]
    assert (other[2] != res[2]).sum() >= 3


def test_subsets_for_the_cell_count_and_work_list_cases_exist():
    recs, tables, refs, walked, (res, counts, d) = rm.cached("crafted")
    for n in (0, 1, 2, 3, 63, 64, 65):
        rm.pick_records(np.diff(walked[0]).astype(np.int64), n)
    per_record = np.bincount(d["record"][d["undecided"]], minlength=len(recs))
    need = np.bincount(d["record"][d["in_bounds"]], minlength=len(recs)) > 0
    for n in (0, 1, 65):
        assert len(rm.pick_records(per_record, n, need=need)) >= 5


# ---- bindings and driver --------------------------------------------------------------------------------------------------------------------------
def test_new_ctypes_mirrors_match_the_header_layout(tmp_path):
    """sizeof / offsetof of floria_ref_seqs and floria_realign_counts, measured by gcc, equal the mirrors in floria_amd/_capi.py"""
    from floria_amd import _capi as capi
    pairs = {"floria_ref_seqs": capi.CRefSeqs, "floria_realign_counts": capi.CRealignCounts}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "floria_hip.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f}));' for f, _ in cls._fields_]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    for line in subprocess.check_output([str(tmp_path / "layout")], text=True).strip().splitlines():
        name, size, *offs = line.split()
        cls = pairs[name]
        assert int(size) == C.sizeof(cls), name
        assert [int(o) for o in offs] == [getattr(cls, f).offset for f, _ in cls._fields_], name


def test_the_library_exports_the_new_entry_point(hip_lib):
    assert "floria_hip_pileup_records_realign" in hip_lib.SYMBOLS
    so = os.path.join(ROOT, "floria_amd", "csrc", "libfloria_hip.so")
    assert hasattr(C.CDLL(so), "floria_hip_pileup_records_realign")


def test_the_driver_knows_pileup_fused(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pileup host|device|fused" in r.stderr
    # the value passes the grammar: what stops this run is the missing BAM
    r = subprocess.run([floria_hip, "-b", str(tmp_path / "none.bam"), "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--pileup", "fused"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pileup takes" not in r.stderr and "none.bam" in r.stderr
    r = subprocess.run([floria_hip, "-b", "x.bam", "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--pileup", "fusion"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pileup takes host or device" in r.stderr and "fused" in r.stderr and "fusion" in r.stderr
