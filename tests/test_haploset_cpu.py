"""`-m "not gpu"`: the model of S2's epilogue (tests/haploset_model.py: assign -> groups -> splits -> sort) against the oracle and against hand-computed cases, the scan
form the kernels of csrc/haploset_kernel.h use against the two walks it replaces, the random generator's share of splits, and floria-hip's --haplosets flag as far
as it needs no device."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import haploset_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
SEED_FIRST, N_RANDOM = 0, 300      # the random contigs of tests/test_gpu_haplosets.py: haploset_model.random_contig(seed) for seed in 0 .. 299


def _first_last(spans):
    return np.array([s[0] for s in spans], np.uint32), np.array([s[1] for s in spans], np.uint32)


def _disjoint(groups):
    seen, out = set(), []
    for g in groups:
        out.append([r for r in g if r not in seen])
        seen.update(g)
    return out


HAND_EXPECT = {
    # name -> (groups, ranges) after the epilogue, worked out by hand from part_block_manip.rs:27-98 and :276-288
    "one_gap": ([[0, 1], [], [3]], [(1, 4), (1, 10), (5, 10)]),                      # read 2, the first behind the gap, is in neither part
    "two_gaps": ([[0, 1], [], [3], [5]], [(1, 4), (1, 20), (5, 10), (11, 20)]),
    "latest_eq_hi": ([[0, 1]], [(1, 4)]),
    "latest_eq_lo": ([[0], [], []], [(4, 4), (4, 12), (5, 12)]),
    "latest_lt_lo": ([[0, 1]], [(5, 12)]),
    "bridge": ([[0, 1, 2, 3]], [(1, 40)]),
    "empty_group": ([[0, 1], []], [(1, 4), (2, 9)]),
    "stable": ([[2], [0], [1], [], []], [(1, 4), (1, 6), (1, 6), (1, 10), (5, 10)]),
    "part_between": ([[1], [0], [], [], [3]], [(1, 3), (1, 4), (1, 10), (5, 10), (6, 9)]),
}


@pytest.mark.parametrize("name", sorted(HAND_EXPECT))
def test_model_hand_cases(name):
    spans, groups, ranges = hm.hand_cases()[name]
    f, l = _first_last(spans)
    assert hm.epilogue(f, l, groups, ranges) == HAND_EXPECT[name]
    assert hm.epilogue_scan(f, l, groups, ranges) == HAND_EXPECT[name]
    assert hm.epilogue(f, l, groups, ranges, assign_only=True) == ([list(g) for g in groups], [tuple(r) for r in ranges])


@pytest.mark.parametrize("name", sorted(hm.hand_cases()))
def test_model_matches_oracle_on_hand_cases(name):
    """Disjoint groups: every read has one candidate, the re-insertion puts it there, and the oracle's result is the epilogue of the input groups."""
    spans, groups, ranges = hm.hand_cases()[name]
    p = hm.reads_pileup(spans)
    f, l = _first_last(spans)
    parts, rng = hm.epilogue(f, l, groups, ranges)
    got = oracle.reassign(p, groups, ranges, 0.03125)
    assert got.n_groups == len(parts)
    assert [list(map(int, got.group(g))) for g in range(got.n_groups)] == parts
    assert [tuple(map(int, r)) for r in got.range] == rng


def test_tile_cases_split_where_the_tile_ends():
    for n, at in ((64, 63), (65, 64), (129, 63), (129, 64), (129, 128)):
        spans, groups, ranges = hm.hand_cases()[f"tile_{n}_{at}"]
        f, l = _first_last(spans)
        parts, _ = hm.epilogue(f, l, groups, ranges)
        assert parts == [list(range(at)), [], list(range(at + 1, n))]      # read `at`, the first behind the gap, is dropped


def test_scan_form_equals_the_two_walks_and_the_oracle_on_random_contigs():
    """The hint of the issue, proven: breaks ascend strictly, so the reads the second walk drops are the reads a break was recorded at."""
    n_split = 0
    for seed in range(SEED_FIRST, SEED_FIRST + N_RANDOM):
        spans, groups, ranges = hm.random_contig(seed)
        f, l = _first_last(spans)
        groups = _disjoint(groups)
        a = hm.epilogue(f, l, groups, ranges)
        assert a == hm.epilogue_scan(f, l, groups, ranges), seed
        n_split += hm.n_splits(f, l, groups, ranges) > 0
        if seed % 10 == 0:                                             # the oracle on every tenth (it builds a pileup per contig)
            got = oracle.reassign(hm.reads_pileup(spans), groups, ranges, 0.03125)
            assert ([list(map(int, got.group(g))) for g in range(got.n_groups)], [tuple(map(int, r)) for r in got.range]) == a, seed
    assert n_split * 5 > N_RANDOM, n_split                             # splits are common: more than one contig in five has one


def test_scan_form_on_adversarial_walks():
    """Reads in arbitrary (not Frag::cmp) order, zeros, equal values, ranges that cut the breaks: the identity does not rest on the sort order of the reads."""
    rng = np.random.default_rng(7)
    for _ in range(400):
        n = int(rng.integers(0, 40))
        f = rng.integers(0, 30, n)
        l = f + rng.integers(0, 6, n)
        lo = int(rng.integers(0, 20)); hi = int(rng.integers(lo, 40))
        ids = list(range(n))
        cut = int(rng.integers(0, n + 1))
        groups, ranges = [ids[:cut], ids[cut:]], [(lo, hi), (int(rng.integers(0, 10)), int(rng.integers(10, 40)))]
        assert hm.epilogue(f, l, groups, ranges) == hm.epilogue_scan(f, l, groups, ranges)


def test_groups_from_assign():
    assert hm.groups_from_assign([1, -1, 0, 1, 2, 0], 4) == [[2, 5], [0, 3], [4], []]


@pytest.fixture(scope="module")
def floria_hip():
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def test_usage_names_the_haplosets_flag(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--haplosets host|resident" in r.stderr and "floria_hip_reassign_batch_resident" in r.stderr and "Any --pileup route" in r.stderr


def test_unknown_haplosets_value_is_refused(floria_hip):
    r = subprocess.run([floria_hip, "-b", "x.bam", "-v", "x.vcf", "-r", "x.fa", "--haplosets", "device"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--haplosets takes host or resident, not 'device'" in r.stderr


def test_header_python_and_rust_sketch_name_the_new_symbols():
    from floria_amd import lib
    new = ["floria_hip_reassign_batch_resident", "floria_hip_haplosets_free", "floria_hip_haplosets_download", "floria_hip_haploset_stats_resident",
           "floria_hip_hapq_batch_resident", "floria_hip_haploset_alleles_resident", "floria_hip_read_spans_resident"]
    header = open(os.path.join(ROOT, "include", "floria_hip.h")).read()
    sketch = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in new:
        assert s + "(" in header and s in lib.SYMBOLS and "pub fn " + s + "(" in sketch, s
