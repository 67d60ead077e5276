"""`-m gpu`: floria_hip_pileup_records_realign (csrc/realign_gather_kernel.h + the realign kernels) against the model of tests/pileup_realign_model.py, its
refusals, and floria-hip --pileup fused against --pileup host on the same inputs (same fragments, same files)."""
import os
import re

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import pileup_model as pm
from tests import pileup_realign_model as rm
from tests.test_gpu_pileup import FIELDS, hand_built, run_route

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
COUNTS = ("cells", "in_bounds", "shortcut", "scored", "changed")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    import subprocess
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def device_realign(ctx, records, tables, refs, walk=None, pad=lambda i: i % 4):
    off, seq = rm.pack_refs(refs)
    return ctx.pileup_records_realign(**pm.pack_records(records, pad=pad), **pm.pack_tables(tables), ref_off=off, ref_seq=seq, walk=walk)


def assert_equal(got, want, want_counts, what=""):
    res, counts = got
    assert len(res) == 6
    for name, g, w in zip(FIELDS, res, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} places, the first at {int(bad[0])}: {int(g[bad[0]])} instead of {int(w[bad[0]])}")
    assert counts == want_counts, (what, counts, want_counts)


def slice_of(model, order):
    """the model's result and counts for the records `order` of the case the model was computed for (every cell is decided on its own)"""
    (cell_off, snp, allele, qual, seq_pos, ref_end), _, d = model
    walked_allele = d["walked_allele"]
    sel = np.concatenate([np.arange(int(cell_off[i]), int(cell_off[i + 1])) for i in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    off = np.zeros(len(order) + 1, np.uint64)
    off[1:] = np.cumsum([int(cell_off[i + 1] - cell_off[i]) for i in order])
    counts = dict(cells=len(sel), in_bounds=int(d["in_bounds"][sel].sum()), shortcut=int(d["decided"][sel].sum()), scored=int(d["undecided"][sel].sum()),
                  changed=int((allele[sel] != walked_allele[sel]).sum()))
    return (off, snp[sel], allele[sel], qual[sel], seq_pos[sel], ref_end[np.asarray(order, np.int64)]), counts


def test_crafted_case_equals_the_model(gpu_ctx):
    recs, tables, refs, walked, model = rm.cached("crafted")
    want, counts, d = model
    assert counts["scored"] > 100 and counts["shortcut"] > 100 and counts["changed"] > 100 and counts["cells"] - counts["in_bounds"] > 100
    assert_equal(device_realign(gpu_ctx, recs, tables, refs), want, counts, "all records")
    t = gpu_ctx.timing()
    assert t["total_ms"] > 0 and t["h2d_ms"] > 0 and t["d2h_ms"] > 0 and t["pileup_ms"] > 0
    # the walk alone is what it was: the realigned call changes alleles only
    plain = gpu_ctx.pileup_records(**pm.pack_records(recs, pad=lambda i: i % 4), **pm.pack_tables(tables))
    for name, g, w in zip(FIELDS, plain, walked):
        assert np.array_equal(g, w), name
    # every record as the only one of a call, and all of them in reverse order
    for i in range(len(recs)):
        w, c = slice_of(model, [i])
        assert_equal(device_realign(gpu_ctx, [recs[i]], tables, refs), w, c, f"record {i} alone")
    order = list(range(len(recs)))[::-1]
    w, c = slice_of(model, order)
    assert_equal(device_realign(gpu_ctx, rm.subset(recs, order), tables, refs), w, c, "reverse order")
    # the contig without a reference: its cells come back as walked
    no_ref = np.isin(d["record"], [i for i, r in enumerate(recs) if r["contig"] == 2])
    assert no_ref.sum() >= 3 and np.array_equal(want[2][no_ref], walked[2][no_ref])


@pytest.mark.parametrize("n_cells", [0, 1, 2, 3, 63, 64, 65])
def test_cell_counts_around_a_half_and_a_whole_wavefront(gpu_ctx, n_cells):
    recs, tables, refs, walked, model = rm.cached("crafted")
    order = rm.pick_records(np.diff(walked[0]).astype(np.int64), n_cells)
    w, c = slice_of(model, order)
    assert c["cells"] == n_cells and len(order) >= min(n_cells, 1)
    assert_equal(device_realign(gpu_ctx, rm.subset(recs, order), tables, refs), w, c, f"{n_cells} cells")


@pytest.mark.parametrize("n_windows", [0, 1, 65])
def test_work_lists_of_no_one_and_65_windows(gpu_ctx, n_windows):
    recs, tables, refs, walked, model = rm.cached("crafted")
    d = model[2]
    per_record = np.bincount(d["record"][d["undecided"]], minlength=len(recs))
    order = rm.pick_records(per_record, n_windows, need=np.bincount(d["record"][d["in_bounds"]], minlength=len(recs)) > 0)
    w, c = slice_of(model, order)
    assert c["scored"] == n_windows and c["in_bounds"] > n_windows and len(order) >= 5
    assert_equal(device_realign(gpu_ctx, rm.subset(recs, order), tables, refs), w, c, f"{n_windows} windows")


def test_more_cells_than_one_pass_of_the_gather_grid_and_more_windows_than_one_pass_of_the_scoring_grid(gpu_ctx):
    """256 CUs: the gather kernels take 8 cells per workgroup and at most 8 workgroups per CU in one pass (16 384 cells), the exact DP 4 windows per workgroup and at
    most 32 workgroups per CU (32 768 windows)"""
    recs, tables, refs = rm.sweep_case(seed=77, n_records=2700, sub_rate=0.12, hidden_indel=0.35, supp=0.15)
    want, counts, _ = rm.realign_records(recs, tables, refs, use_shortcut=True)
    print(counts)
    assert counts["cells"] > 2 * 16384 and counts["scored"] > 32768
    assert_equal(device_realign(gpu_ctx, recs, tables, refs), want, counts, "large case")


@pytest.mark.parametrize("member", [None, (8, 0, 0), (1, 1, 1)], ids=["exact", "8,max,right", "1,sum,down"])
def test_sweep_equals_the_model_from_pageable_and_pinned_memory(gpu_ctx, member):
    recs, tables, refs, walked, (want, counts, d) = rm.cached("sweep", member)
    print(counts)
    assert counts["scored"] >= 1000 and counts["shortcut"] >= 1000 and counts["cells"] - counts["in_bounds"] >= 200 and counts["changed"] >= 200
    assert_equal(device_realign(gpu_ctx, recs, tables, refs, walk=member), want, counts, "pageable")
    from floria_amd import lib
    packed, tab = pm.pack_records(recs, pad=lambda i: i % 4), pm.pack_tables(tables)
    off, seq = rm.pack_refs(refs)
    packed["ref_seq"] = seq
    arena = lib.PinnedArena(sum(v.nbytes for v in packed.values()) + 8192)
    pinned = {}
    for k, v in packed.items():
        pinned[k] = arena.take(v.size, v.dtype)
        pinned[k][:] = v
    assert_equal(gpu_ctx.pileup_records_realign(**pinned, **tab, ref_off=off, walk=member), want, counts, "pinned")
    assert gpu_ctx.timing()["upload_pinned_bytes"] >= packed["blob"].nbytes + seq.nbytes
    del pinned
    arena.free()


def test_contigs_with_empty_references_come_back_as_walked(gpu_ctx):
    recs, tables, refs, walked, model = rm.cached("crafted")
    n = int(walked[0][-1])
    none = dict(cells=n, in_bounds=0, shortcut=0, scored=0, changed=0)
    assert_equal(device_realign(gpu_ctx, recs, tables, [b""] * len(refs)), walked, none, "no reference at all")
    packed, tab = pm.pack_records(recs), pm.pack_tables(tables)
    got = gpu_ctx.pileup_records_realign(**packed, **tab, ref_off=np.zeros(len(refs) + 1, np.uint64), ref_seq=None)          # (a null pointer is fine when nothing is there)
    assert_equal(got, walked, none, "null seq, empty contigs")
    # only the middle contig has a reference
    some = [b"", refs[1], b""]
    want, counts, _ = rm.realign_records(recs, tables, some, walked=walked)
    assert 0 < counts["in_bounds"] < model[1]["in_bounds"]
    assert_equal(device_realign(gpu_ctx, recs, tables, some), want, counts, "one contig of three")


def test_bad_references_and_walk_members_are_refused_by_the_host_part(gpu_ctx, hip_lib):
    recs, tables, refs, walked, model = rm.cached("crafted")
    order = list(range(0, len(recs), 7))
    recs = rm.subset(recs, order)
    want, counts = slice_of(model, order)
    packed, tab = pm.pack_records(recs), pm.pack_tables(tables)
    off, seq = rm.pack_refs(refs)

    def refused(word, ref_off=off, ref_seq=seq, walk=None):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.pileup_records_realign(**packed, **tab, ref_off=ref_off, ref_seq=ref_seq, walk=walk)
        assert ei.value.code == -1 and word in str(ei.value), str(ei.value)
        assert_equal(gpu_ctx.pileup_records_realign(**packed, **tab, ref_off=off, ref_seq=seq), want, counts, "after the refusal")      # the context still serves a valid call

    refused("contigs", ref_off=off[:-1])                                                  # one contig fewer than the SNP table
    refused("contigs", ref_off=np.concatenate([off, off[-1:]]))                           # ... one more
    dec = off.copy(); dec[1], dec[2] = off[2], off[1]
    refused("decreases", ref_off=dec)
    refused("null seq", ref_seq=None)
    refused("floria_realign_walk", walk=(3, 0, 0))                                         # no such step
    refused("floria_realign_walk", walk=(16, 8, 0, 0))                                     # no such block
    refused("floria_realign_walk", walk=(8, 2, 0))
    refused("floria_realign_walk", walk=(8, 0, 2))


# ---- floria-hip --pileup fused against --pileup host ------------------------------------------------------------------------------------------
FUSED_LINE = re.compile(r"Realignment: (\d+) calls scored on the device behind the walk \((\d+) by the exact shortcut, (\d+) outside the window bounds\), scoring (.+)")


def fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=(), eps_list=(0.03125, 0.04)):
    """the two routes write to the SAME output directory one after the other (its path is part of every vartig header) -> the fused runs' stderr"""
    errs = []
    for eps in eps_list:
        out, dump = str(tmp_path / "out"), str(tmp_path / "frags.txt")
        host_tree, host_dump, _ = run_route(floria_hip, prefix, out, dump, "host", eps, extra)
        dev_tree, dev_dump, err = run_route(floria_hip, prefix, out, dump, "fused", eps, extra)
        assert "Pileup on the device:" in err and FUSED_LINE.search(err) and len(host_dump) > 1000
        assert dev_dump == host_dump, f"--dump-frags differs at -e {eps}"
        assert sorted(dev_tree) == sorted(host_tree) and len(host_tree) >= 4
        for fn in host_tree:
            assert dev_tree[fn] == host_tree[fn], f"{fn} differs at -e {eps}"
        errs.append(err)
    return errs


def test_cli_noisy_long_reads_and_the_undecided_set_of_the_device_route(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 1, 0.6, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12, realign=False)
    errs = fused_agrees_with_host(floria_hip, tmp_path, prefix)
    _, _, dev_err = run_route(floria_hip, prefix, str(tmp_path / "out"), str(tmp_path / "frags.txt"), "device", 0.04, ())
    n_device = int(re.search(r"Realignment: (\d+) calls scored on the device in", dev_err).group(1))
    for err in errs:
        m = FUSED_LINE.search(err)
        assert int(m.group(1)) == n_device > 1000 and int(m.group(2)) > 1000 and m.group(4).strip() == "exact affine-gap DP"
        assert "calls scored on the device in" not in err                        # nothing went through the host's queue


def test_cli_noisy_long_reads_scored_by_a_fixed_block_walk(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 1, 0.6, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12, realign=False)
    for err in fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--realign", "block:8,max,right")):
        m = FUSED_LINE.search(err)
        assert int(m.group(1)) > 1000 and m.group(4).strip() == "fixed-block walk block:8,max,right"


def test_cli_paired_short_reads(floria_hip, tmp_path):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.03, realign=False)
    fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("-l", "500"))


def test_cli_edited_cigars_with_output_reads(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 0, 0.5, keep_layout=True)
    prefix = str(tmp_path / "l")
    synth_bam.write_dataset(prefix, [c], seed=7, edit_frac=0.5, sub_rate=0.05, realign=False)
    fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--output-reads",))


def test_cli_supplementary_pairs(floria_hip, tmp_path):
    prefix = str(tmp_path / "h")
    hand_built(prefix)
    fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--snp-count-filter", "10", "--supp-aln-dist-cutoff", "10000", "--output-reads"))


def test_cli_batches_of_contigs_and_bam_segments(floria_hip, tmp_path):
    cs = [synth.make_config_contig(4, 20 + i, 0.25 + 0.02 * i, keep_layout=True) for i in range(8)] + [synth.make_config_contig(3, 5, 0.2, keep_layout=True)]
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, cs, seed=7, edit_frac=0.5, sub_rate=0.05, realign=False)
    fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--batch-contigs", "3"), eps_list=(0.03125,))
    for err in fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--bam-window-kb", "64", "-t", "1"), eps_list=(0.04,)):
        assert int(re.search(r"BAM: \d+ records in (\d+) segments", err).group(1)) > 1
        assert int(re.search(r"Pileup on the device: \d+ records, \d+ blob bytes in (\d+) calls", err).group(1)) > 1


def test_cli_contig_with_a_five_allele_site_falls_back_and_says_so(floria_hip, tmp_path):
    prefix = str(tmp_path / "h")
    hand_built(prefix, five_alleles=True)
    for err in fused_agrees_with_host(floria_hip, tmp_path, prefix, extra=("--snp-count-filter", "10")):
        assert err.count("keeps the host walk") == 1 and "--pileup fused: contig c " in err
        assert "Pileup on the device: 0 records" in err and int(FUSED_LINE.search(err).group(1)) == 0


def test_cli_fused_without_realignment_is_the_device_route(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 1, 0.3, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12, realign=False)
    out, dump = str(tmp_path / "out"), str(tmp_path / "frags.txt")
    _, dev_dump, dev_err = run_route(floria_hip, prefix, out, dump, "device", 0.04, ("--no-realign", "--ingest-only"))
    _, fus_dump, fus_err = run_route(floria_hip, prefix, out, dump, "fused", 0.04, ("--no-realign", "--ingest-only"))
    assert fus_dump == dev_dump and len(dev_dump) > 1000 and "behind the walk" not in fus_err and "Pileup on the device:" in fus_err
    # --ingest-only with the realignment: the device realigns (fused), the host threads do (host)
    _, host_dump, _ = run_route(floria_hip, prefix, out, dump, "host", 0.04, ("--ingest-only",))
    _, fus_dump, fus_err = run_route(floria_hip, prefix, out, dump, "fused", 0.04, ("--ingest-only",))
    assert fus_dump == host_dump and host_dump != dev_dump and int(FUSED_LINE.search(fus_err).group(1)) > 100


def test_a_realigning_call_ends_the_residency_of_an_s1_batch(gpu_ctx, hip_lib):
    """the work list of the realignment lives where the partitions of the last S1 batch do: floria_hip_hap_graph must refuse that batch afterwards (host validation,
    nothing reaches a kernel), while floria_hip_pileup_records, which does not use that buffer, leaves the batch resident as before"""
    c = synth.make_config_contig(4, 0, scale=0.4)
    s, e = hip_lib.get_range_with_lengths(c.snp_pos, 10000)
    recs, tables, refs, walked, model = rm.cached("crafted")
    d = model[2]
    order = rm.pick_records(np.bincount(d["record"][d["undecided"]], minlength=len(recs)), 65)
    want, counts = slice_of(model, order)
    assert counts["scored"] == 65
    sub = rm.subset(recs, order)
    contig = gpu_ctx.upload(c.pileup)
    try:
        def phase():
            return gpu_ctx.phase_blocks_batch([contig], np.zeros(len(s), np.uint32), s, e, hip_lib.make_params(0.03125))
        r = phase()
        g0 = gpu_ctx.hap_graph(r)
        r = phase()
        plain = gpu_ctx.pileup_records(**pm.pack_records(sub), **pm.pack_tables(tables))
        assert np.array_equal(plain[0], want[0])
        g1 = gpu_ctx.hap_graph(r)                                               # still resident after the plain walk
        assert np.array_equal(g0.node_cov.view(np.uint64), g1.node_cov.view(np.uint64)) and np.array_equal(g0.edge_w, g1.edge_w)
        r = phase()
        assert_equal(device_realign(gpu_ctx, sub, tables, refs, pad=lambda i: 0), want, counts, "between phase_blocks and hap_graph")
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.hap_graph(r)
        assert ei.value.code == -1 and "no longer resident" in str(ei.value), str(ei.value)
        r = phase()                                                             # the context goes on serving
        g2 = gpu_ctx.hap_graph(r)
        assert np.array_equal(g0.node_cov.view(np.uint64), g2.node_cov.view(np.uint64)) and np.array_equal(g0.edge_w, g2.edge_w)
    finally:
        contig.free()
