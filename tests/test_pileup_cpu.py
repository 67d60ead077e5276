"""`-m "not gpu"`: the yardstick of the device pileup (tests/pileup_model.py) is pinned to the product's host route, the shared test inputs can tell
wrong walks from the right one, and the driver knows --pileup."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import pileup_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def host_route(floria_hip, prefix, tmp_path, extra=()):
    from tests.test_gpu_cli import parse_frag_dump
    dump = prefix + ".frags"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-e", "0.03", "-l", "10000",
                        "--ingest-only", "--no-realign", "--dump-frags", dump, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return parse_frag_dump(dump)


def assert_model_is_the_host_route(got, records, table):
    """got: one contig of parse_frag_dump; records: name -> model record (single-alignment reads)"""
    seen = set()
    for g in got["reads"]:
        m = pm.walk_record(records[g["name"]], table)
        assert g["cells"] == list(zip(m["snp"], m["allele"], m["qual"])), g["name"]
        assert (g["first"], g["last"]) == (m["snp"][0], m["snp"][-1]) and g["span"] == (records[g["name"]]["pos"], m["ref_end"]), g["name"]
        seen.add(g["name"])
    for name, span, _len in got["snpless"]:
        m = pm.walk_record(records[name], table)
        assert m["snp"] == [] and span == (records[name]["pos"], m["ref_end"]), name
        seen.add(name)
    assert seen == set(records)
    return len(got["reads"])


def test_model_reproduces_the_host_walk_on_long_reads_with_edited_cigars(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 0, 1.0, keep_layout=True)
    prefix = str(tmp_path / "d")
    ex = synth_bam.write_dataset(prefix, [c], seed=23, edit_frac=0.5, realign=False)[c.name]
    table = pm.read_vcf_tables(prefix + ".vcf", [c.name])[c.name]
    assert np.array_equal(table.pos, ex["snp_pos0"].astype(np.int64))
    records = {}
    for name, alns in ex["read_alignments"].items():
        assert len(alns) == 1
        pos, seq, cig, qual = alns[0]
        records[name] = dict(pos=pos, flag=0, cigar=cig, seq=seq, qual=np.frombuffer(qual, np.uint8))
    assert sum(1 for r in records.values() if len(r["cigar"]) > 1) > len(records) // 4             # the edited CIGARs are there
    n = assert_model_is_the_host_route(host_route(floria_hip, prefix, tmp_path)[c.name], records, table)
    assert n > 100


def hand_built_files(prefix):
    """BAM / VCF / FASTA of the crafted records of contig 0 that a BAM of single primary alignments can hold -> (records by name, SnpTable)"""
    recs, tables = pm.crafted_case()
    recs = sorted((r for r in recs if r["contig"] == 0 and not r["flag"] & 0x800 and r["pos"] >= 0), key=lambda r: r["pos"])
    t = tables[0]
    clen = 6000
    ref = synth_bam.BASES[np.random.default_rng(3).integers(0, 4, size=clen)]
    with open(prefix + ".fa", "w") as f:
        f.write(">h\n" + bytes(ref).decode() + "\n")
    with open(prefix + ".vcf", "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=h,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" % clen)
        for p, al, na in zip(t.pos, t.alleles, t.n_alleles):
            f.write("h\t%d\t.\t%s\t%s\t50\tPASS\t.\n" % (p + 1, chr(al[0]), ",".join(chr(x) for x in al[1:na]) if na > 1 else "."))
    synth_bam.write_bam(prefix + ".bam", [("h", clen)], [r["raw"] for r in recs])
    return {r["name"]: r for r in recs}, t


def test_model_reproduces_the_host_walk_on_a_hand_built_bam_with_every_cigar_op(floria_hip, tmp_path):
    prefix = str(tmp_path / "h")
    records, table = hand_built_files(prefix)
    assert set(op for r in records.values() for op, _ in r["cigar"]) == set(pm.OPS)
    file_table = pm.read_vcf_tables(prefix + ".vcf", ["h"])["h"]
    used = np.arange(4)[None, :] < table.n_alleles[:, None]                         # (the crafted table keeps a byte behind a one-allele site: a walk must not read it)
    assert np.array_equal(file_table.pos, table.pos) and np.array_equal(file_table.n_alleles, table.n_alleles) and np.array_equal(file_table.alleles[used], table.alleles[used])
    n = assert_model_is_the_host_route(host_route(floria_hip, prefix, tmp_path)["h"], records, table)
    assert n >= 15


def test_the_shared_inputs_tell_wrong_walks_from_the_right_one():
    for recs, tables in (pm.crafted_case(), pm.random_case(n_records=3000)):
        right = pm.walk_records(recs, tables)
        with_cells = sum(1 for i in range(len(recs)) if right[0][i + 1] > right[0][i])
        assert len(pm.changed_records(right, pm.walk_records(recs, tables, seq_pos_off=1))) >= (with_cells + 1) // 2
        assert len(pm.changed_records(right, pm.walk_records(recs, tables, n_like_m=True))) >= 1
        assert len(pm.changed_records(right, pm.walk_records(recs, tables, ignore_hard_clip=True))) >= 1


def test_the_random_sweep_is_not_thin():
    """the caps tests/test_gpu_pileup.py asserts before it compares, met by the generator with the model alone"""
    recs, tables = pm.random_case()
    cov = pm.coverage(recs, tables, pm.walk_records(recs, tables))
    assert len(recs) >= 20000 and len(tables) == 3 and cov["ops"] == set(pm.OPS)
    assert cov["cells"] >= 10000 and cov["under_dn"] >= 100 and cov["long_records"] >= 100
    packed = pm.pack_records(recs[:64], pad=lambda i: i % 4)
    assert set((packed["cigar_off"] % 4).tolist()) == {0, 1, 2, 3}


def test_crafted_records_cover_what_they_claim():
    recs, tables = pm.crafted_case()
    assert {len(r["cigar"]) for r in recs} >= {63, 64, 65, 129} and max(len(r["cigar"]) for r in recs) >= 5000
    assert {int(t.n_alleles[k]) for t in tables for k in range(len(t.pos))} >= {1, 2, 3, 4}
    assert any(r["cigar"] == [("M", 5000)] and np.count_nonzero((tables[r["contig"]].pos >= r["pos"]) & (tables[r["contig"]].pos < r["pos"] + 5000)) >= 200 for r in recs)
    assert any(len(r["seq"]) == 0 and r["cigar"] for r in recs) and any(r["qual"].size and (r["qual"] == 255).all() for r in recs)
    assert {r["contig"] for r in recs} == {0, 1}


def test_unknown_pileup_route_is_refused(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "-b", "x.bam", "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--pileup", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "host" in r.stderr and "device" in r.stderr and "bogus" in r.stderr


def test_help_lists_the_pileup_flag(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pileup host|device" in r.stderr


def test_new_ctypes_mirrors_match_the_header_layout(tmp_path):
    """sizeof / offsetof of the three structs of floria_hip_pileup_records, measured by gcc, equal the mirrors in floria_amd/_capi.py"""
    from floria_amd import _capi as capi
    pairs = {"floria_alignments": capi.CAlignments, "floria_snp_table": capi.CSnpTable, "floria_record_cells": capi.CRecordCells, "floria_timing": capi.CTiming}
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
