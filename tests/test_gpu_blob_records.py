"""`-m gpu`: floria_hip_blob_records (csrc/inflate_kernel.h: the chain walk and the per-record pass) against a plain parse of the downloaded blob."""
import struct

import numpy as np
import pytest

from floria_amd import synth_bam
from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu

FIELDS = ("offset", "block_size", "ref_id", "pos", "l_seq", "cigar0", "flag", "n_cigar_op", "mapq", "l_read_name")


def to_blob(ctx, raw, member_bytes=7001):
    """raw bytes -> BGZF members of member_bytes inflated bytes each -> the device blob (records straddle the members)"""
    members = [ic.bgzf_member(ic.deflate(raw[o:o + member_bytes], 6)) for o in range(0, len(raw), member_bytes)]
    off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64) if members else np.zeros(0, np.uint64)
    return ctx.inflate_bgzf(b"".join(members), off, [len(m) for m in members])


def parse(raw, begin, end):
    """the model: follow the block_size prefixes of every chain through the DOWNLOADED bytes"""
    cols = {f: [] for f in FIELDS}
    names, rec_off, stop = [], [0], []
    for b, e in zip(begin, end):
        o = int(b)
        while o < e:
            bs, = struct.unpack_from("<I", raw, o)
            assert bs >= 32 and o + 4 + bs <= e
            ref_id, pos, lrn, mapq, _bin, nco, flag, l_seq = struct.unpack_from("<iiBBHHHI", raw, o + 4)
            cg = o + 36 + lrn
            for f, v in zip(FIELDS, (o, bs, ref_id, pos, l_seq, struct.unpack_from("<I", raw, cg)[0] if nco else 0, flag, nco, mapq, lrn)):
                cols[f].append(v)
            names.append(raw[o + 36:o + 36 + lrn])
            o += 4 + bs
        rec_off.append(len(names)); stop.append(o)
    return cols, names, rec_off, stop


def check(ctx, raw_records, begin, end, member_bytes=7001):
    blob = to_blob(ctx, raw_records, member_bytes)
    try:
        raw = blob.download().tobytes()
        assert raw == raw_records
        got = ctx.blob_records(blob, begin, end)
    finally:
        blob.free()
    cols, names, rec_off, stop = parse(raw, begin, end)
    assert got["chain_rec_off"].tolist() == rec_off and got["chain_stop"].tolist() == stop
    for f in FIELDS:
        assert got[f].tolist() == cols[f], f
    no = got["name_off"]
    assert no[0] == 0 and np.all(np.diff(no.astype(np.int64)) == got["l_read_name"]) and int(no[-1]) == len(got["names"])
    assert [got["names"][int(no[i]):int(no[i + 1])].tobytes() for i in range(len(names))] == names
    return got


def records(n, seed=4, name=lambda i: f"read{i}"):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 700))
        cigar = [("S", 3), ("M", ln)] if i % 3 == 0 else [("M", ln + 3)]
        out.append(synth_bam.bam_record(int(i % 2), 100 + 17 * i, name(i), int(rng.integers(0, 4096)), int(rng.integers(0, 61)), cigar,
                                        bytes(synth_bam.BASES[rng.integers(0, 4, size=ln + 3)]), rng.integers(5, 41, size=ln + 3).astype(np.uint8)))
    return out


def test_zero_records_and_one_record(gpu_ctx):
    one = records(1)[0]
    got = check(gpu_ctx, one, [0], [0])                                   # an empty chain
    assert len(got["offset"]) == 0 and got["chain_stop"].tolist() == [0]
    got = check(gpu_ctx, one, [0], [len(one)])
    assert len(got["offset"]) == 1
    got = check(gpu_ctx, one, [], [])                                     # no chain at all
    assert len(got["offset"]) == 0 and len(got["chain_rec_off"]) == 1
    t = gpu_ctx.timing()
    assert t["total_ms"] == 0 and t["pileup_ms"] == 0


def test_names_of_1_and_254_characters(gpu_ctx):
    recs = records(5, name=lambda i: ("x" if i % 2 == 0 else "n" * 254))
    raw = b"".join(recs)
    got = check(gpu_ctx, raw, [0], [len(raw)])
    assert sorted(set(got["l_read_name"].tolist())) == [2, 255]
    assert gpu_ctx.timing()["pileup_ms"] > 0


def test_three_chains_of_different_lengths_each_ending_exactly_at_end(gpu_ctx):
    recs = records(700)
    raw = b"".join(recs)
    cuts = np.cumsum([0] + [len(r) for r in recs])
    begin = [int(cuts[0]), int(cuts[3]), int(cuts[250])]
    end = [int(cuts[3]), int(cuts[250]), int(cuts[700])]
    got = check(gpu_ctx, raw, begin, end)
    assert got["chain_rec_off"].tolist() == [0, 3, 250, 700] and got["chain_stop"].tolist() == end
    # the same chains in another order, with a gap: a chain need not begin where another ends
    check(gpu_ctx, raw, [int(cuts[600]), int(cuts[0]), int(cuts[10])], [int(cuts[700]), int(cuts[7]), int(cuts[300])])
    # more chains than one workgroup of the chain kernel holds: one chain per record
    check(gpu_ctx, raw, cuts[:-1].tolist(), cuts[1:].tolist())


def test_malformed_chains_are_refused_with_chain_and_offset(gpu_ctx, hip_lib):
    recs = records(40)
    cuts = np.cumsum([0] + [len(r) for r in recs])
    raw = b"".join(recs)

    def refused(raw_bytes, begin, end, word, chain, offset):
        blob = to_blob(gpu_ctx, raw_bytes)
        try:
            with pytest.raises(hip_lib.FloriaHipError) as ei:
                gpu_ctx.blob_records(blob, begin, end)
            assert ei.value.code == -1 and f"chain {chain} " in str(ei.value) and f"offset {offset}:" in str(ei.value) and word in str(ei.value), str(ei.value)
            good = gpu_ctx.blob_records(blob, [0], [int(cuts[10])])       # the context and the blob still serve a good call
            assert len(good["offset"]) == 10
        finally:
            blob.free()
    short = bytearray(raw)
    short[int(cuts[20]):int(cuts[20]) + 4] = struct.pack("<I", 31)
    refused(bytes(short), [0, int(cuts[12])], [int(cuts[12]), len(raw)], "block_size below", 1, int(cuts[20]))
    refused(raw, [0, int(cuts[5])], [int(cuts[5]), int(cuts[30]) - 1], "runs past", 1, int(cuts[29]))      # the last record is cut by one byte
    refused(raw, [0], [int(cuts[30]) + 2], "runs past", 0, int(cuts[30]))                                  # ... and a block_size prefix cut in two
    blob = to_blob(gpu_ctx, raw)
    for b, e in (([5], [4]), ([0], [len(raw) + 1])):
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.blob_records(blob, b, e)
        assert ei.value.code == -1 and "chain 0" in str(ei.value)
    other = hip_lib.FloriaHip(0)
    with pytest.raises(hip_lib.FloriaHipError) as ei:
        other.blob_records(blob, [0], [len(raw)])
    assert ei.value.code == -1 and "another context" in str(ei.value)
    other.close()
    blob.free()


def test_first_cigar_word_of_a_cg_tag_record(gpu_ctx):
    """a record with more than 65 535 operations as the specification writes it: the placeholder kSmN in the field, the real CIGAR in CG:B,I"""
    from tests.test_host_cpu import _bam_record
    cigar = [("M", 1), ("I", 1)] * 35000 + [("M", 5)]
    l_seq = 70005
    ref_len = 35005
    rng = np.random.default_rng(6)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, size=l_seq))
    recs = [_bam_record(0, 50, "plain", 0, 60, [("M", 20)], "ACGT" * 5, [30] * 20),
            _bam_record(0, 80, "long_cigar", 0, 60, cigar, seq, [25] * l_seq, real_cigar_in_cg=True),
            _bam_record(-1, -1, "unmapped", 4, 0, [], "ACGTACGT", [20] * 8)]
    raw = b"".join(recs)
    got = check(gpu_ctx, raw, [0], [len(raw)], member_bytes=65280)
    assert got["n_cigar_op"].tolist() == [1, 2, 0]
    assert got["cigar0"].tolist() == [20 << 4, (l_seq << 4) | 4, 0]       # kSmN: the first word is l_seq soft-clipped
    assert got["ref_id"].tolist() == [0, 0, -1] and got["block_size"][1] > 4 * 70001 and ref_len == sum(n for op, n in cigar if op == "M")
