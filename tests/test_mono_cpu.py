"""CPU tests of the --ignore-monomorphic model (tests/mono_model.py) that floria_hip_drop_monomorphic is compared with on the device: against the C++ host's own
restatement of utils_frags.rs:713-772 on an ingest dump, on a hand case with one site of every rule, and the two new exports of the library."""
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from floria_amd.pileup import Pileup
from tests import mono_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "floria-hip")


def dump(floria_hip, prefix, tmp_path, extra):
    from tests.test_gpu_cli import parse_frag_dump
    path = prefix + ".frags"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-l", "10000",
                        "--ingest-only", "--dump-frags", path, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return parse_frag_dump(path)


def test_model_equals_the_host_filter_on_an_ingest_dump(floria_hip, tmp_path):
    eps = 0.03125
    c = synth.make_config_contig(1, 0, keep_layout=True)
    prefix = str(tmp_path / "d")
    ex = synth_bam.write_dataset(prefix, [c], seed=5, realign=False)[c.name]
    plain = dump(floria_hip, prefix, tmp_path, ("--no-realign", "-e", str(eps)))[c.name]["reads"]
    filt = dump(floria_hip, prefix, tmp_path, ("--no-realign", "-e", str(eps), "--ignore-monomorphic"))[c.name]["reads"]
    # the plain dump is in Frag::cmp order: its rows are the pileup's reads
    cells = [g["cells"] for g in plain]
    off = np.zeros(len(cells) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in cells])
    flat = np.array([t for x in cells for t in x], np.int64).reshape(-1, 3)
    p = Pileup(off, flat[:, 0].astype(np.uint32), flat[:, 1].astype(np.uint8), flat[:, 2].astype(np.uint8),
               np.array([g["first"] for g in plain], np.uint32), np.array([g["last"] for g in plain], np.uint32))
    n_snps = len(ex["snp_pos0"])
    assert int(p.snp.max()) <= n_snps
    q, old_read, removed = mm.drop_monomorphic(p, n_snps, eps)
    assert 0 < int(removed.sum()) < n_snps and q.n_cells < p.n_cells
    assert q.n_reads == len(filt)
    assert [plain[int(i)]["name"] for i in old_read] == [g["name"] for g in filt]
    for r, g in enumerate(filt):
        s, a, ql = q.read(r)
        assert list(zip(s.tolist(), a.tolist(), ql.tolist())) == g["cells"], f"read {r}"
    assert q.first.tolist() == [g["first"] for g in filt] and q.last.tolist() == [g["last"] for g in filt]
    assert not np.array_equal(old_read, np.sort(old_read)), "the re-sort must have moved a read"


def test_hand_case_has_one_site_of_every_rule():
    p = mm.hand_pileup()
    w = float(mm.phred_scale([10])[0])
    assert (2 * w) * mm.HAND_ERROR == w and float(mm.phred_scale([9])[0]) < w and float(mm.phred_scale([0])[0]) == 0.0
    mask = mm.removed_mask(p, mm.HAND_SNPS, mm.HAND_ERROR)
    assert np.array_equal(mask, mm.HAND_MASK)
    alleles = lambda s: sorted(set(p.allele[p.snp == s].tolist()))
    assert alleles(1) == [0] and mask[0] == 1                                            # one allele
    assert alleles(2) == [0, 1] and mask[1] == 0                                         # v0 * error == v1: kept
    assert alleles(3) == [0, 1] and mask[2] == 1                                         # just below: removed
    assert set(p.qual[(p.snp == 4) & (p.allele == 1)].tolist()) == {0} and mask[3] == 1  # the minor allele only at q = 0: a key all the same
    assert alleles(5) == [0, 1, 2] and mask[4] == 0                                      # three alleles
    assert not (p.snp == 6).any() and mask[5] == 0 and not (p.snp == 9).any() and mask[8] == 0      # nobody calls it
    # without the q = 0 key SNP 4 would have one allele: removed either way; with a one-allele SNP whose only cells weigh 0 the key alone removes it
    z = Pileup.from_reads([([1, 2], [0, 0], [0, 20]), ([1, 2], [0, 1], [0, 20])])
    assert mm.removed_mask(z, 2, 0.5).tolist() == [1, 0]
    q, old_read, _ = mm.drop_monomorphic(p, mm.HAND_SNPS, mm.HAND_ERROR)
    assert p.n_reads - q.n_reads == 1                                                    # a read dropped entirely
    assert not np.array_equal(old_read, np.sort(old_read))                               # a trimmed first moved a read behind a later one
    same = [(r, r + 1) for r in range(q.n_reads - 1) if (q.first[r], q.last[r]) == (q.first[r + 1], q.last[r + 1])]
    assert same and all(old_read[a] < old_read[b] for a, b in same)                      # equal (first, last): the old index decides
    assert any(q.first[r] == q.first[r + 1] and q.last[r] > q.last[r + 1] for r in range(q.n_reads - 1))
    assert not mask[q.snp.astype(np.int64) - 1].any()
    # the set order of a cut-down read: the old order with the removed cells deleted, renumbered
    assert mm.filter_set_order([1, 2, 3, 5, 8], [4, 0, 2, 1, 3], mm.HAND_MASK).tolist() == [2, 0, 1]


def test_filter_set_order_on_a_long_read_equals_a_list_with_the_removed_keys_deleted():
    """the model tests/test_gpu_chain_trips.py holds mono_order_kernel against, on a read of 290 cells with a random order: a `remove` moves no other key, so the
    filtered order is the old one without the removed cells, each renamed to its rank among the survivors — stated here with plain lists"""
    rng = np.random.default_rng(12)
    snps = np.sort(rng.choice(np.arange(1, 301), size=290, replace=False))
    order = rng.permutation(290)
    removed = (rng.random(300) < 0.3).astype(np.uint8)
    alive = [int(s) for s in snps if not removed[s - 1]]
    want = [alive.index(int(snps[i])) for i in order if not removed[int(snps[i]) - 1]]
    assert len(want) > 128 and len(want) < 290
    got = mm.filter_set_order(snps, order, removed)
    assert got.dtype == np.uint32 and got.tolist() == want and sorted(want) == list(range(len(alive)))


def test_library_exports_the_entry_points(hip_lib):
    import ctypes
    L = ctypes.CDLL(os.path.join(ROOT, "floria_amd", "csrc", "libfloria_hip.so"))
    for s in ("floria_hip_drop_monomorphic", "floria_hip_mono_result_free", "floria_hip_mono_timing"):
        assert hasattr(L, s) and s in hip_lib.SYMBOLS, s
