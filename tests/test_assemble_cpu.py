"""`-m "not gpu"`: the model of floria_hip_assemble_contigs (tests/assemble_model.py) against a plain-dict restatement of combine_frags, and the ctypes mirrors
of the structs the feature adds against gcc's layout of the header."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import assemble_model as am
from tests import pileup_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_world(seed, n_records=400, n_snps=60):
    """records with random cells on two contigs -> (records, tables, walked)"""
    rng = np.random.default_rng(seed)
    tables = [am.grid_table(n_snps), am.grid_table(n_snps // 2, start=57, step=7)]
    recs = []
    for i in range(n_records):
        c = int(rng.integers(0, 2))
        n = len(tables[c].pos)
        lo = int(rng.integers(1, n + 1)); hi = min(n, lo + int(rng.integers(0, 25)))
        snps = [s for s in range(lo, hi + 1) if rng.random() < 0.7] if rng.random() < 0.92 else []
        recs.append(am.record_with(tables[c], {s: (int(rng.integers(0, 4)), int(rng.integers(0, 60))) for s in snps}, contig=c, name="w%d" % i))
    return recs, tables, pm.walk_records(recs, tables)


def random_fragments(rng, recs, walked, contig, n_frags):
    """lists of 1..4 records of the contig (any order, repeats allowed), each with at least one cell in some part"""
    mine = [i for i, r in enumerate(recs) if r["contig"] == contig]
    full = [i for i in mine if walked[0][i + 1] > walked[0][i]]
    out = []
    for _ in range(n_frags):
        k = int(rng.choice([1, 1, 1, 2, 2, 3, 4]))
        f = [int(rng.choice(mine)) for _ in range(k)]
        f[int(rng.integers(0, k))] = int(rng.choice(full))
        out.append(f)
    return out


def dict_fragment(recs, tables, parts):
    """combine_frags as the reference states it: seq_dict / qual_dict of the base record, `extend`ed by every later record"""
    seq, qual = {}, {}
    for i in parts:
        o = pm.walk_record(recs[i], tables[recs[i]["contig"]])
        seq.update(dict(zip(o["snp"], o["allele"]))); qual.update(dict(zip(o["snp"], o["qual"])))
    keys = sorted(seq)
    return keys, [seq[k] for k in keys], [qual[k] for k in keys], min(keys), max(keys)


def test_model_equals_the_dict_restatement():
    recs, tables, walked = random_world(11)
    rng = np.random.default_rng(12)
    frags = [random_fragments(rng, recs, walked, c, 150) for c in (0, 1)]
    plan = am.build_plan(walked, frags)
    overwritten = 0
    for c in (0, 1):
        want = [dict_fragment(recs, tables, f) for f in frags[c]]
        order = sorted(range(len(want)), key=lambda k: (want[k][3], -want[k][4], k))          # Frag::cmp with counter_id = the place in the list
        assert list(plan["order"][c]) == order
        p = plan["pileups"][c]
        assert p.n_reads == len(order) and int(plan["frag_off"][c + 1] - plan["frag_off"][c]) == len(order)
        for r, k in enumerate(order):
            s, a, q = p.read(r)
            assert (list(s), list(a), list(q)) == want[k][:3]
            assert (int(p.first[r]), int(p.last[r])) == want[k][3:]
            f = int(plan["frag_off"][c]) + r
            assert list(plan["part_rec"][int(plan["part_off"][f]):int(plan["part_off"][f + 1])]) == frags[c][k]
            overwritten += sum(len(am.record_cells(walked, i)[0]) for i in frags[c][k]) - len(s)
    assert overwritten > 200          # the inputs do overlap: "later overwrites" was exercised


def test_set_orders_of_the_plan_and_of_the_pileups_are_the_same_permutations():
    recs, tables, walked = random_world(13, n_records=80)
    rng = np.random.default_rng(14)
    plan = am.build_plan(walked, [random_fragments(rng, recs, walked, c, 20) for c in (0, 1)], set_order_rng=np.random.default_rng(15))
    assert np.array_equal(plan["set_order"], np.concatenate([p.set_order for p in plan["pileups"]]))
    for p in plan["pileups"]:
        for r in range(p.n_reads):
            lo, hi = int(p.read_off[r]), int(p.read_off[r + 1])
            assert sorted(p.set_order[lo:hi]) == list(range(hi - lo))


def test_new_ctypes_mirrors_match_the_header_layout(tmp_path):
    """as test_ctypes_mirrors_match_the_header_layout, for floria_record_summary and floria_fragment_plan (nested fields by their first member)"""
    from floria_amd import _capi as capi
    pairs = {"floria_record_summary": capi.CRecordSummary, "floria_fragment_plan": capi.CFragmentPlan, "floria_realign_counts": capi.CRealignCounts}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "floria_hip.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {f}));')
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    assert len(out) == len(pairs)
    for line in out:
        name, size, *offs = line.split()
        cls = pairs[name]
        assert int(size) == C.sizeof(cls), f"{name}: header {size} B, ctypes {C.sizeof(cls)} B"
        assert [int(o) for o in offs] == [getattr(cls, f).offset for f, _ in cls._fields_], name
