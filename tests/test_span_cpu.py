"""CPU tests of the read-position model (tests/span_model.py) that the device is compared with in tests/test_gpu_spans.py: against a plain-dict restatement of
`snp_pos_to_seq_pos.extend` on the hand cases, against the C++ host's own maps on ingest dumps (floria-hip --ingest-only --dump-seq-pos) for a paired short-read
contig and a long-read contig with and without --ignore-monomorphic, and the two new exports of the library."""
import os
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from floria_amd.pileup import Pileup
from tests import assemble_model as am
from tests import mono_model as mm
from tests import pileup_model as pm
from tests import span_model as sm
from tests.test_gpu_assemble import HAND, hand_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")


# ---- the dictionary restatement ---------------------------------------------------------------------------------------------------------------------------------
def dict_merge(walked, parts, mates):
    """combine_frags as the reference writes it: every part's map `extend`s the fragment's (dict.update: the later entry overwrites)"""
    d = {}
    for i, m in zip(parts, mates):
        a, b = int(walked[0][i]), int(walked[0][i + 1])
        d.update({int(s): (int(m), int(p)) for s, p in zip(walked[1][a:b], walked[4][a:b])})
    return sorted(d.items())


@pytest.mark.parametrize("name", sorted(HAND))
def test_merge_equals_a_dict_update_restatement(name):
    recs, walked, frags = hand_world([name])
    parts = frags[0]
    mates = [0] + [1] * (len(parts) - 1)
    snp, _, _, w = sm.merge_seq_pos(walked, parts, mates)
    want = dict_merge(walked, parts, mates)
    assert [(int(s), (int(x) >> 31, int(x) & 0x7fffffff)) for s, x in zip(snp, w)] == want
    s3 = am.merge_fragment(walked, parts)
    assert np.array_equal(snp, s3[0])
    # a cell's seq_pos is its genome offset in its record: parts that share a SNP disagree about it
    if name == "two_identical_sets":
        b = int(walked[0][parts[1]]), int(walked[0][parts[1] + 1])
        assert np.array_equal(w, sm.word(1, walked[4][b[0]:b[1]])), "only the second part's positions, with mate 1"
    if name == "same_record_twice":
        assert (w >> 31).all(), "the third part (the first record again, marked as the second mate) overwrites what it shares and keeps the rest of the second's"
    if name in ("two_boundary_overlap", "three_share_one", "against_genome_order"):
        first = {int(s): int(p) for s, p in zip(*[walked[k][int(walked[0][parts[0]]):int(walked[0][parts[0] + 1])] for k in (1, 4)])}
        later = {int(s) for i in parts[1:] for s in walked[1][int(walked[0][i]):int(walked[0][i + 1])]}
        shared = sorted(set(first) & later)
        assert shared and all(dict(want)[s][0] == 1 for s in shared), "the later part wins the SNPs both have"
        if name == "two_boundary_overlap":          # the records start at different bases: the parts disagree about the position, and the later one's stands
            assert all(dict(want)[s][1] != first[s] for s in shared)


def test_identical_sets_yield_the_later_part_whichever_it_is():
    recs, walked, frags = hand_world(["two_identical_sets"])
    p0, p1 = frags[0]
    a, b = walked[4][int(walked[0][p0]):int(walked[0][p0 + 1])], walked[4][int(walked[0][p1]):int(walked[0][p1 + 1])]
    assert len(a) == len(b) == 40
    snp, _, _, w = sm.merge_seq_pos(walked, [p0, p1], [0, 1])
    assert np.array_equal(w & 0x7fffffff, b) and (w >> 31 == 1).all()
    snp, _, _, w = sm.merge_seq_pos(walked, [p1, p0], None)
    assert np.array_equal(w, a)


def test_query_model_on_a_small_read():
    p = Pileup.from_reads([([3, 5, 9], [0, 1, 0], [30, 30, 30])])
    w = [np.array([10, 20, 0x80000000 | 30], np.uint32)]
    q = lambda lo, hi: tuple(int(x[0]) for x in sm.read_spans([p], w, [0], [[0]], [(lo, hi)]))
    assert q(1, 20) == (10, 0x8000001e) and q(3, 9) == (10, 0x8000001e) and q(4, 8) == (20, 20) and q(6, 8) == (0x8000001e, 20)
    assert q(10, 12) == (sm.NONE, 0x8000001e) and q(1, 2) == (10, sm.NONE) and q(9, 3) == (0x8000001e, 10)


# ---- the C++ host -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "floria-hip")


def parse_seq_pos_dump(path):
    """-> {contig: [(fragment id, [(snp, mate, seq_pos)])]}"""
    contigs, cur = {}, None
    for line in open(path):
        t = line.rstrip("\n").split("\t")
        if t[0] == "#CONTIG":
            cur = contigs.setdefault(t[1], [])
        else:
            cur.append((t[0], [tuple(int(x) for x in c.split(":")) for c in t[1:]]))
    return contigs


def dump_seq_pos(floria_hip, prefix, tmp_path, extra):
    path = prefix + ".seqpos"
    r = subprocess.run([floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", str(tmp_path / "unused"), "-l", "10000",
                        "--ingest-only", "--dump-seq-pos", path, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return parse_seq_pos_dump(path)


def model_of_dataset(prefix, c, ex):
    """the model's fragments of a synth_bam data set, in the pileup's order: every read's alignments as records (first in pair, then its mate), walked against the
    VCF's table and merged -> (Pileup, words, names)"""
    table = pm.read_vcf_tables(prefix + ".vcf", [c.name])[c.name]
    recs, frags, mates = [], [], []
    for nm in ex["names"]:
        al = ex["read_alignments"][nm]
        frags.append(list(range(len(recs), len(recs) + len(al))))
        mates.append(list(range(len(al))))                                             # 0 for the first in pair / the only alignment, 1 for its mate
        recs += [pm.make_record(pos, cig, seq, np.frombuffer(q, np.uint8), name=nm) for pos, seq, cig, q in al]
    walked = pm.walk_records(recs, [table])
    merged = [sm.merge_seq_pos(walked, f, m) for f, m in zip(frags, mates)]
    off = np.zeros(len(merged) + 1, np.uint32)
    off[1:] = np.cumsum([len(m[0]) for m in merged])
    cat = lambda j, dt: np.concatenate([m[j] for m in merged]).astype(dt)
    p = Pileup(off, cat(0, np.uint32), cat(1, np.uint8), cat(2, np.uint8), np.array([m[0][0] for m in merged], np.uint32), np.array([m[0][-1] for m in merged], np.uint32))
    return p, cat(3, np.uint32), list(ex["names"])


def rows_of(p, words, names):
    return [(nm, [(int(s), int(w) >> 31, int(w) & 0x7fffffff) for s, w in zip(p.read(r)[0], words[int(p.read_off[r]):int(p.read_off[r + 1])])]) for r, nm in enumerate(names)]


def test_model_equals_the_host_maps_of_a_paired_contig(floria_hip, tmp_path):
    c = synth.make_config_contig(3, 2, 0.2, keep_layout=True)
    prefix = str(tmp_path / "d")
    ex = synth_bam.write_dataset(prefix, [c], seed=3, realign=False)[c.name]
    assert ex["paired"]
    got = dump_seq_pos(floria_hip, prefix, tmp_path, ("--no-realign",))[c.name]
    p, words, names = model_of_dataset(prefix, c, ex)
    assert np.array_equal(p.snp, ex["pileup"].snp) and np.array_equal(p.read_off, ex["pileup"].read_off)
    assert (words >> 31 == 0).any() and (words >> 31 == 1).any(), "cells of both mates"
    assert got == rows_of(p, words, names)


def test_model_equals_the_host_maps_of_a_long_read_contig_with_and_without_the_filter(floria_hip, tmp_path):
    eps = 0.03125
    c = synth.make_config_contig(1, 0, keep_layout=True)
    prefix = str(tmp_path / "d")
    ex = synth_bam.write_dataset(prefix, [c], seed=5, realign=False)[c.name]
    plain = dump_seq_pos(floria_hip, prefix, tmp_path, ("--no-realign", "-e", str(eps)))[c.name]
    filt = dump_seq_pos(floria_hip, prefix, tmp_path, ("--no-realign", "-e", str(eps), "--ignore-monomorphic"))[c.name]
    p, words, names = model_of_dataset(prefix, c, ex)
    assert np.array_equal(p.snp, ex["pileup"].snp)
    assert plain == rows_of(p, words, names)
    cells_in = [(s, w) for _, row in plain for s, _, w in row]
    assert any(True for _ in cells_in) and not (words >> 31).any()
    # (reads with a soft clip, an insertion and deletions: seq_pos is not the genome offset in the record)
    n_snps = len(ex["snp_pos0"])
    q, fwords = sm.filter_words(p, words, n_snps, eps)
    _, old_read, removed = mm.drop_monomorphic(p, n_snps, eps)
    assert 0 < int(removed.sum()) < n_snps and q.n_cells < p.n_cells and not np.array_equal(old_read, np.sort(old_read))
    assert filt == rows_of(q, fwords, [names[int(i)] for i in old_read])


def test_library_exports_the_entry_points(hip_lib):
    import ctypes
    L = ctypes.CDLL(os.path.join(ROOT, "floria_amd", "csrc", "libfloria_hip.so"))
    for s in ("floria_hip_assemble_contigs_opt", "floria_hip_read_spans"):
        assert hasattr(L, s) and s in hip_lib.SYMBOLS, s
