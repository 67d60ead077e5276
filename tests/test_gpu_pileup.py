"""`-m gpu`: floria_hip_pileup_records (csrc/pileup_kernel.h) against the model of tests/pileup_model.py, its refusals, and floria-hip --pileup device against
--pileup host on the same inputs (same fragments, same files)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from floria_amd import synth, synth_bam
from tests import pileup_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")
FIELDS = ("cell_off", "snp", "allele", "qual", "seq_pos", "ref_end")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def device_walk(ctx, records, tables, pad=lambda i: i % 4):
    return ctx.pileup_records(**pm.pack_records(records, pad=pad), **pm.pack_tables(tables))


def assert_equal_results(got, want, records):
    assert len(got) == 6
    for name, g, w in zip(FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
    bad = pm.changed_records(want, got) if np.array_equal(got[0], want[0]) else [int(np.nonzero(got[0] != want[0])[0][0]) - 1]
    assert not bad, f"{len(bad)} records differ, the first: #{bad[0]} pos {records[bad[0]]['pos']} flag {records[bad[0]]['flag']} cigar {records[bad[0]]['cigar'][:8]} ({len(records[bad[0]]['cigar'])} ops)"
    for name, g, w in zip(FIELDS, got, want):
        assert np.array_equal(g, w), name


def test_crafted_records_equal_the_model(gpu_ctx):
    recs, tables = pm.crafted_case()
    want = pm.walk_records(recs, tables)
    assert int(want[0][-1]) > 1000
    packed = pm.pack_records(recs, pad=lambda i: i % 4)
    assert set((packed["cigar_off"] % 4).tolist()) == {0, 1, 2, 3}                     # CIGAR words at all four byte alignments
    assert_equal_results(gpu_ctx.pileup_records(**packed, **pm.pack_tables(tables)), want, recs)
    t = gpu_ctx.timing()
    assert t["total_ms"] > 0 and t["h2d_ms"] > 0 and t["d2h_ms"] > 0 and t["pileup_ms"] > 0
    # the same records one by one (every record as the only one of a call) and in reverse order
    for r in recs:
        assert_equal_results(device_walk(gpu_ctx, [r], tables), pm.walk_records([r], tables), [r])
    assert_equal_results(device_walk(gpu_ctx, recs[::-1], tables), pm.walk_records(recs[::-1], tables), recs[::-1])


@pytest.mark.parametrize("n", [0, 1, 65, 4173])
def test_record_counts_that_fill_no_workgroup_wavefront_or_scan_tile(gpu_ctx, n):
    recs, tables = pm.random_case(seed=99, n_records=4173)
    recs = recs[:n]
    assert_equal_results(device_walk(gpu_ctx, recs, tables), pm.walk_records(recs, tables), recs)


def test_random_sweep_equals_the_model(gpu_ctx):
    recs, tables, want = pm.random_sweep()
    cov = pm.coverage(recs, tables, want)
    assert len(recs) >= 20000 and len(tables) == 3 and cov["ops"] == set(pm.OPS), cov
    assert cov["cells"] >= 10000 and cov["under_dn"] >= 100 and cov["long_records"] >= 100, cov
    assert_equal_results(device_walk(gpu_ctx, recs, tables), want, recs)
    # the same from pinned memory (DMA without the staging ring)
    from floria_amd import lib
    packed, tab = pm.pack_records(recs, pad=lambda i: i % 4), pm.pack_tables(tables)
    arena = lib.PinnedArena(sum(v.nbytes for v in packed.values()) + 4096)
    pinned = {}
    for k, v in packed.items():
        pinned[k] = arena.take(v.size, v.dtype)
        pinned[k][:] = v
    assert_equal_results(gpu_ctx.pileup_records(**pinned, **tab), want, recs)
    assert gpu_ctx.timing()["upload_pinned_bytes"] >= packed["blob"].nbytes
    del pinned
    arena.free()


def test_malformed_input_is_refused_by_the_host_part(gpu_ctx, hip_lib):
    recs, tables = pm.crafted_case()
    recs = recs[:12]
    want = pm.walk_records(recs, tables)
    good_r, good_t = pm.pack_records(recs), pm.pack_tables(tables)
    blob_bytes = good_r["blob"].size

    def refused(code, word, rec=None, tab=None):
        r = {k: v.copy() for k, v in good_r.items()}
        t = {k: v.copy() for k, v in good_t.items()}
        (rec or (lambda r: None))(r); (tab or (lambda t: None))(t)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.pileup_records(**r, **t)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        assert_equal_results(gpu_ctx.pileup_records(**good_r, **good_t), want, recs)         # the context still serves a valid call

    def put(key, i, value):
        def f(d):
            d[key][i] = value
        return f
    refused(-1, "CIGAR", rec=put("cigar_off", 3, blob_bytes - 3))                          # an offset range past blob_bytes
    refused(-1, "CIGAR", rec=put("n_cigar", 3, 0x7fffffff))
    refused(-1, "sequence", rec=put("seq_off", 0, blob_bytes))
    refused(-1, "quality", rec=put("qual_off", 5, 2 ** 63))
    refused(-1, "contig", rec=put("contig", 7, 2))                                         # contig out of range
    refused(-1, "ascending", tab=put("snp_pos", 11, int(good_t["snp_pos"][10])))           # not strictly ascending (equal)
    refused(-1, "ascending", tab=put("snp_pos", 450, 0))                                   # ... decreasing, in the second contig
    refused(-1, "n_alleles", tab=put("n_alleles", 20, 0))
    refused(-4, "alleles", tab=put("n_alleles", 20, 5))


# ---- floria-hip --pileup device against --pileup host ----------------------------------------------------------------------------------------
def run_route(floria_hip, prefix, out, dump, route, eps, extra):
    if os.path.exists(out):
        shutil.rmtree(out)
    cmd = [floria_hip, "-b", prefix + ".bam", "-v", prefix + ".vcf", "-r", prefix + ".fa", "-o", out, "-e", repr(eps), "-l", "10000", "-t", "4",
           "--dump-frags", dump, "--pileup", route, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    tree = {}
    for dp, _, fs in os.walk(out):
        for f in fs:
            if f != "cmd.log":
                tree[os.path.relpath(os.path.join(dp, f), out)] = open(os.path.join(dp, f), "rb").read()
    return tree, open(dump).read(), r.stderr


def both_routes_agree(floria_hip, tmp_path, prefix, extra=(), eps_list=(0.03125, 0.04)):
    """the two routes write to the SAME output directory one after the other (its path is part of every vartig header)"""
    errs = []
    for eps in eps_list:
        out, dump = str(tmp_path / "out"), str(tmp_path / "frags.txt")
        host_tree, host_dump, _ = run_route(floria_hip, prefix, out, dump, "host", eps, extra)
        dev_tree, dev_dump, err = run_route(floria_hip, prefix, out, dump, "device", eps, extra)
        assert "Pileup on the device:" in err and len(host_dump) > 1000
        assert dev_dump == host_dump, f"--dump-frags differs at -e {eps}"
        assert sorted(dev_tree) == sorted(host_tree) and len(host_tree) >= 4
        for fn in host_tree:
            assert dev_tree[fn] == host_tree[fn], f"{fn} differs at -e {eps}"
        errs.append(err)
    return errs


def test_cli_long_reads_with_edited_cigars(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 0, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, edit_frac=0.5)
    both_routes_agree(floria_hip, tmp_path, prefix)


def test_cli_noisy_reads_where_realignment_consumes_seq_pos(floria_hip, tmp_path):
    c = synth.make_config_contig(1, 1, 0.6, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7, sub_rate=0.12)
    for err in both_routes_agree(floria_hip, tmp_path, prefix):
        import re
        assert int(re.search(r"Realignment: (\d+) calls scored on the device", err).group(1)) > 1000


def test_cli_paired_short_reads_and_output_reads(floria_hip, tmp_path):
    c = synth.make_config_contig(3, 2, 0.3, keep_layout=True)
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, [c], seed=7)
    both_routes_agree(floria_hip, tmp_path, prefix, extra=("-l", "500"))
    both_routes_agree(floria_hip, tmp_path, prefix, extra=("-l", "500", "--output-reads"))
    c = synth.make_config_contig(1, 0, 0.5, keep_layout=True)
    prefix = str(tmp_path / "l")
    synth_bam.write_dataset(prefix, [c], seed=7, edit_frac=0.5)
    both_routes_agree(floria_hip, tmp_path, prefix, extra=("--output-reads",))


def test_cli_batches_of_contigs_and_bam_segments(floria_hip, tmp_path):
    cs = [synth.make_config_contig(4, 20 + i, 0.25 + 0.02 * i, keep_layout=True) for i in range(8)] + [synth.make_config_contig(3, 5, 0.2, keep_layout=True)]
    prefix = str(tmp_path / "d")
    synth_bam.write_dataset(prefix, cs, seed=7, edit_frac=0.5)
    both_routes_agree(floria_hip, tmp_path, prefix, extra=("--batch-contigs", "3"))
    for err in both_routes_agree(floria_hip, tmp_path, prefix, extra=("--bam-window-kb", "64", "-t", "1")):
        import re
        assert int(re.search(r"BAM: \d+ records in (\d+) segments", err).group(1)) > 1


def hand_built(prefix, five_alleles=False):
    """one contig, SNPs every 500 bases: plain reads over everything (so that there is something to phase), a primary + supplementary pair whose pieces lie within
    --supp-aln-dist-cutoff 10000 (merged; the supplementary piece is hard-clipped, its seq_pos shifted) and one beyond it (the primary alone)"""
    rng = np.random.default_rng(5)
    clen = 60000
    ref = synth_bam.BASES[rng.integers(0, 4, size=clen)].copy()
    snp_pos = 1000 + 500 * np.arange(100)
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    alt = np.array([nxt[int(ref[q])] for q in snp_pos], np.uint8)
    with open(prefix + ".fa", "w") as f:
        f.write(">c\n" + bytes(ref).decode() + "\n")
    with open(prefix + ".vcf", "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=c,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n" % clen)
        for i, q in enumerate(snp_pos):
            a = chr(alt[i])
            if five_alleles and i == 30:
                a = ",".join(chr(x) for x in (alt[i], nxt[int(alt[i])], nxt[nxt[int(alt[i])]], ref[q]))         # REF + four ALTs (one repeats REF): five alleles
            f.write(f"c\t{q + 1}\t.\t{chr(ref[q])}\t{a}\t50\tPASS\t.\tGT\t0/1\n")
    recs = []

    def add(name, pos, flag, cigar, hap):                       # (no leading soft clip, no indels: query offset = reference offset)
        n = sum(ln for op, ln in cigar if op in pm.Q_OPS)
        s = ref[pos:pos + n].copy()
        for i, q in enumerate(snp_pos):
            if pos <= q < pos + n and hap[i % len(hap)]:
                s[q - pos] = alt[i]
        recs.append((pos, synth_bam.bam_record(0, pos, name, flag, 60, cigar, bytes(s), rng.integers(10, 40, size=n).astype(np.uint8))))
    haps = ([0, 1, 1, 0, 1], [1, 0, 0, 1, 0, 1, 1])
    for k in range(240):
        pos = int(rng.integers(200, clen - 9000))
        add(f"plain{k}", pos, 0, [("M", 8000)], haps[k % 2])
    add("supp_near", 20900, 0, [("M", 1200), ("S", 700)], haps[0])
    add("supp_near", 24900, 2048, [("H", 1200), ("M", 700)], haps[0])
    add("supp_far", 30900, 0, [("M", 700)], haps[1])
    add("supp_far", 900, 2048, [("H", 300), ("M", 700)], haps[1])
    recs.sort(key=lambda t: t[0])
    synth_bam.write_bam(prefix + ".bam", [("c", clen)], [r for _, r in recs])


def test_cli_supplementary_pairs_within_and_beyond_the_distance_cutoff(floria_hip, tmp_path):
    prefix = str(tmp_path / "h")
    hand_built(prefix)
    extra = ("--snp-count-filter", "10", "--supp-aln-dist-cutoff", "10000", "--output-reads")
    both_routes_agree(floria_hip, tmp_path, prefix, extra=extra)
    from tests.test_gpu_cli import parse_frag_dump
    reads = {g["name"]: g for g in parse_frag_dump(str(tmp_path / "frags.txt"))["c"]["reads"]}
    assert reads["supp_near"]["span"] == (20900, 22100) and reads["supp_near"]["last"] >= 49 and reads["supp_far"]["first"] >= 60


def test_cli_contig_with_a_five_allele_site_keeps_the_host_walk_and_says_so(floria_hip, tmp_path):
    prefix = str(tmp_path / "h")
    hand_built(prefix, five_alleles=True)
    for err in both_routes_agree(floria_hip, tmp_path, prefix, extra=("--snp-count-filter", "10", "--no-realign")):
        assert err.count("keeps the host walk") == 1 and "contig c " in err
        assert "Pileup on the device: 0 records" in err
