"""(no GPU) every case of tests/test_gpu_opt_limits.py, built here from the same code (tests/opt_limits_cases.py) and checked to be what its name says: the launch plan
the library makes for it (tests/opt_plan_model.py), the ploidies the reference tries (the oracle), and the optimise rounds its jobs run (tests/opt_delta_model.py, which
is pinned to oracle.one_ploidy on every job it restates here).  So no GPU case can pass on a path it does not name, and the cases whose seeds were searched for keep the
property they were searched for."""
import os
import re

import numpy as np
import pytest

from tests import opt_limits_cases as cases
from tests import opt_plan_model as pm
from tests.test_gpu_opt_packed import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def phased(oracle, spec):
    """the oracle's result per contig -> (Case, ploidies tried per block); every block holds every read of its contig"""
    c = Case(oracle, spec.pileups, spec.blocks(), P=spec.P)
    for i, p in enumerate(spec.pileups):
        assert int(np.diff(c.oracle[i].read_off.astype(np.int64))[0]) == p.n_reads, (spec.name, i)
    return c, [int(c.oracle[i].ploidies_tried[0]) for i in range(len(spec.pileups))]


def flags(pl, key):
    return {p for p, v in pl.items() if v[key]}


# ---- the plan model itself -------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_model_uses_the_constants_of_the_sources():
    kernel = open(os.path.join(ROOT, "floria_amd", "csrc", "optimize_kernel.h")).read()
    host = open(os.path.join(ROOT, "floria_amd", "csrc", "floria_hip.hip")).read()
    assert int(re.search(r"constexpr int OPT_SORT_LDS = (\d+);", kernel).group(1)) == pm.OPT_SORT_LDS
    assert int(re.search(r"constexpr int OPT_META_MAX = (\d+);", kernel).group(1)) == pm.OPT_META_MAX
    assert "meta_n * 12 + 15" in kernel and pm.META_BYTES_PER_READ == 12
    rule = re.search(r"q\.hl = hist_bytes \+ \(size_t\)span_max \* p \+ 32 \+ moved_bytes \+ meta_bytes <= (\d+) \* 1024", host)
    assert rule and int(rule.group(1)) * 1024 == pm.LDS_BUDGET


def test_the_plan_model_against_figures_worked_out_by_hand():
    # 100 reads: one bit per read in 4 words = 16 bytes, 1 200 bytes of metadata; 61 440 - 32 - 16 - 1 200 = 60 192 bytes for p * 17 bytes per position
    assert (pm.moved_bytes(100), pm.meta_bytes(100)) == (16, 1200)
    assert [pm.largest_hl_span(100, p) for p in (2, 3, 4, 5)] == [60192 // 34, 60192 // 51, 60192 // 68, 60192 // 85] == [1770, 1180, 885, 708]
    assert pm.is_hl(100, 1180, 2, 3) and not pm.is_hl(100, 1181, 2, 3) and pm.smallest_non_hl_span(100, 3) == 1181
    # 4 096 reads: 512 bytes of bits, 48 KiB of metadata: 11 744 bytes are left; one read more and the metadata stays in HBM
    assert (pm.moved_bytes(4096), pm.meta_bytes(4096)) == (512, 49152)
    assert [pm.largest_hl_span(4096, p) for p in (2, 3)] == [345, 230]
    assert (pm.moved_bytes(4097), pm.meta_bytes(4097)) == (528, 0) and pm.largest_hl_span(4097, 5) == (61440 - 32 - 528) // 85 == 716
    # four alleles: 33 bytes per (position, partition)
    assert pm.largest_hl_span(100, 2, alleles=4) == 60192 // 66
    # the moved bitset is rounded to whole words, then to 16 bytes
    assert [pm.moved_bytes(n) for n in (1, 32, 33, 128, 129)] == [16, 16, 16, 16, 32]
    assert [pm.pow2_at_least(m) for m in (1, 2, 3, 511, 512, 513)] == [1, 2, 4, 512, 512, 1024]
    pl = pm.plan(100, 1180, 2, 5)
    assert flags(pl, "hl") == {1, 2, 3} and flags(pl, "packed") == {1, 2, 3} and flags(pl, "delta") == {1, 2, 3}
    assert flags(pm.plan(100, 1180, 2, 5, opt_threads=1024), "opt_spec") == {1, 2, 3} and not flags(pm.plan(100, 1180, 2, 5, opt_threads=1024), "packed")
    assert not flags(pm.plan(100, 1180, 2, 5, opt_threads=1024), "delta") and not flags(pm.plan(100, 60, 2, 5, opt_threads=128), "opt_spec")
    assert flags(pm.plan(100, 60, 2, 5, opt_packed=0), "delta") == {1, 2, 3, 4, 5} and not flags(pm.plan(100, 60, 2, 5, opt_packed=0), "packed")
    assert not flags(pm.plan(100, 60, 2, 5, all_pk=False), "packed")
    assert flags(pm.plan(100, 60, 2, 7), "opt_spec") == {1, 2, 3, 4, 5} and flags(pm.plan(100, 60, 2, 7), "hl") == set(range(1, 8))
    assert pm.stages(5) == [2, 3, 4, 5] and pm.stages(5, fuse_p1=False) == [1, 2, 3, 4, 5] and pm.stages(1) == [1]
    assert pm.launches(pl, 5) == (4, 2) and pm.launches(pl, 5, fuse_p1=False) == (5, 3)


def test_the_largest_block_of_the_batch_decides_for_every_block():
    narrow, wide = (100, 60), (100, pm.largest_hl_span(100, 2))
    assert pm.call_shape([narrow]) == (100, 60) and pm.call_shape([narrow, wide]) == (100, 1770) and pm.call_shape([(4097, 10), wide]) == (4097, 1770)
    assert flags(pm.plan_for_blocks([narrow], 2, 5), "hl") == {1, 2, 3, 4, 5}
    assert flags(pm.plan_for_blocks([narrow, wide], 2, 5), "hl") == {1, 2}
    assert flags(pm.plan_for_blocks([wide, narrow], 2, 5), "hl") == {1, 2}          # (whatever the order of the contigs)
    # ... in both numbers: a block of many reads on another contig takes the metadata's LDS away from a wide block that had it
    assert flags(pm.plan_for_blocks([wide, (4096, 10)], 2, 5), "hl") == set()


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_blocks_of_more_than_512_reads_have_delta_passes_that_decide_a_late_reads_move(oracle_mod):
    spec = cases.case_a()
    assert [n for n, _ in spec.shapes()] == cases.A_COUNTS and all(s == cases.NARROW for _, s in spec.shapes())
    _, tried = phased(oracle_mod, spec)
    for sub in (spec, spec.sub("the call of the blocks up to 513 reads", [0, 1, 2])):
        pl = sub.plan()
        assert flags(pl, "hl") == flags(pl, "packed") == flags(pl, "delta") == {1, 2, 3, 4, 5}
    passes, fallbacks, acc = cases.predict(oracle_mod, spec, tried, spec.plan())
    print("a: tried", tried, "delta passes", [a["passes"] for a in acc], "fallbacks", [a["fallbacks"] for a in acc])
    for n, t, a, pile in zip(cases.A_COUNTS, tried, acc, spec.pileups):
        assert t >= 3, (n, t)
        if n > 512:
            assert a["passes"] >= 1, n
            assert cases.flip_reaches_read_from(a, 512), f"{n} reads: no delta pass has a flip inside the span of a read of index >= 512"
            assert cases.broken_delta_leaves_oracle(oracle_mod, pile, t, 512), f"{n} reads: a delta pass that stops at read 512 would give the same partitions"
        else:
            assert not cases.broken_delta_leaves_oracle(oracle_mod, pile, t, 512)          # (the sensitivity check itself: nothing to miss here)
    assert sum(a["passes"] for a in acc[:3]) >= 2 and sum(a["fallbacks"] for a in acc) >= 1


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_b_a_delta_pass_follows_a_pool_sorted_round_and_rounds_fall_on_both_sides_of_the_lds_sort(oracle_mod):
    spec = cases.case_b()
    assert all(300 <= n <= 400 for n, _ in spec.shapes())
    _, tried = phased(oracle_mod, spec)
    pl = spec.plan()
    assert flags(pl, "delta") == {1, 2, 3, 4, 5}
    _, _, acc = cases.predict(oracle_mod, spec, tried, pl)
    near = []
    for t, a in zip(tried, acc):
        assert t == 4
        rounds = a["rounds"][4]
        print("b: ploidy 4 rounds (M, flips, next pass, accepted)", [(r["M"], len(r["flips"]), r["pass"], r["accepted"]) for r in rounds])
        assert any(r["accepted"] and r["M2"] > pm.OPT_SORT_LDS and r["pass"] == "delta" for r in rounds), "no delta pass right behind a pool-sorted round"
        assert any(r["accepted"] and r["M2"] <= pm.OPT_SORT_LDS for r in rounds) and any(r["accepted"] and r["M2"] > pm.OPT_SORT_LDS for r in rounds)
        assert all(r["M2"] == pm.pow2_at_least(r["M"]) for r in rounds)
        near += [r["M"] for r in rounds if abs(r["M"] - pm.OPT_SORT_LDS) <= 3]
    # what the construction gives at the edge itself: one round two candidates short of a full LDS sort, one round one candidate past it
    assert sorted(near) == [510, 513], near


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_c_the_largest_hl_span_at_ploidy_3_and_one_snp_more(oracle_mod, extra):
    spec = cases.case_c(extra)
    span = pm.largest_hl_span(cases.C_READS, 3) + extra
    assert spec.shapes() == [(cases.C_READS, span)] and 1100 < span < 1250
    lens = np.diff(spec.pileups[0].read_off.astype(np.int64))
    assert lens.min() >= 20 and lens.max() <= 60
    _, tried = phased(oracle_mod, spec)
    assert tried[0] >= 4, "the reference stops before ploidy 4: no stage of this call would run the HBM-histogram instance on an open block"
    pl = spec.plan()
    assert flags(pl, "hl") == flags(pl, "packed") == flags(pl, "delta") == ({1, 2, 3} if extra == 0 else {1, 2})
    assert pm.launches(pl, spec.P) == (4, 2 if extra == 0 else 1)
    passes, fallbacks, acc = cases.predict(oracle_mod, spec, tried, pl)
    print("c:", spec.name, "tried", tried, "delta passes", passes, "fallbacks", fallbacks, "jobs restated", sorted(acc[0]["rounds"]))
    assert sorted(acc[0]["rounds"]) == ([2, 3] if extra == 0 else [2])          # (the prediction is restricted to the HL ploidies)
    assert passes + fallbacks >= 1


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_d_a_wide_block_on_another_contig_takes_the_packed_instances_from_the_narrow_block(oracle_mod):
    alone, batch = cases.case_d(False), cases.case_d(True)
    assert alone.shapes() == [(cases.D_READS, cases.NARROW)] and batch.shapes() == [(cases.D_READS, cases.NARROW), (cases.D_READS, pm.largest_hl_span(cases.D_READS, 2))]
    assert np.array_equal(alone.pileups[0].snp, batch.pileups[0].snp) and np.array_equal(alone.pileups[0].allele, batch.pileups[0].allele)
    _, tried = phased(oracle_mod, batch)
    assert tried[0] >= 3, "the narrow block stops before a ploidy whose instance the batch changes"
    assert flags(alone.plan(), "packed") == {1, 2, 3, 4, 5} and pm.launches(alone.plan(), 5) == (4, 4)
    assert flags(batch.plan(), "packed") == {1, 2} and pm.launches(batch.plan(), 5) == (4, 1)


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_e_4096_reads_stage_their_metadata_and_4097_do_not(oracle_mod):
    at, past = cases.case_e(4096), cases.case_e(4097)
    assert at.shapes() == [(4096, cases.E_SNPS)] and past.shapes() == [(4097, cases.E_SNPS)]
    for spec in (at, past):
        lens = np.diff(spec.pileups[0].read_off.astype(np.int64))
        assert lens.min() >= 3 and lens.max() <= 6
    _, tried_at = phased(oracle_mod, at)
    _, tried_past = phased(oracle_mod, past)
    assert tried_at[0] >= 3 and tried_past[0] >= 3
    pl = at.plan()
    assert all(v["meta"] for v in pl.values()) and flags(pl, "hl") == flags(pl, "packed") == flags(pl, "delta") == {1, 2} and pm.launches(pl, 5) == (4, 1)
    passes, fallbacks, _ = cases.predict(oracle_mod, at, tried_at, pl)
    print("e: 4096 reads: tried", tried_at, "delta passes", passes, "fallbacks", fallbacks)
    assert passes >= 1
    pl = past.plan()
    assert not any(v["meta"] for v in pl.values()) and flags(pl, "hl") == flags(pl, "packed") == {1, 2, 3, 4, 5} and not flags(pl, "delta")
    assert pm.launches(pl, 5) == (4, 4)


# ---- (f) -------------------------------------------------------------------------------------------------------------------------------------------------
def test_f_four_alleles_take_neither_instance(oracle_mod):
    spec = cases.case_f()
    assert spec.shapes() == [(513, cases.NARROW)] and set(int(x) for x in spec.pileups[0].allele) == {0, 1, 2, 3}
    _, tried = phased(oracle_mod, spec)
    assert tried[0] >= 2
    pl = spec.plan()
    assert flags(pl, "hl") == {1, 2, 3, 4, 5} and not flags(pl, "opt_spec") and not flags(pl, "packed") and not flags(pl, "delta")
    assert pm.launches(pl, 5) == (4, 0)
