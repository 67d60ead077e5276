"""`-m gpu`: floria_hip_inflate_bgzf (csrc/inflate_kernel.h) against zlib, byte for byte: every case of tests/inflate_cases.py as a BGZF member, the malformed members
(FLORIA_E_INVALID with the member and the reason, then a good call on the same context), the header refusals of the host part, and the BGZF of a synth_bam file.
The decoder core has been through the same cases on the CPU under the sanitizers (tests/test_inflate_core_cpu.py) before any of them reaches a GPU."""
import struct
import zlib

import numpy as np
import pytest

from floria_amd import synth_bam
from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu

EOF_MEMBER = synth_bam._bgzf_block(b"")


@pytest.fixture(scope="module")
def valid():
    """(name, member bytes, inflated bytes) of every valid case: zlib is the model, computed once"""
    return [(name, ic.bgzf_member(p), zlib.decompress(p, -15)) for name, p, _, _ in ic.valid_cases()]


def inflate(ctx, members):
    """members back to back as one file image -> the downloaded blob"""
    image = b"".join(members)
    off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64) if members else np.zeros(0, np.uint64)
    blob = ctx.inflate_bgzf(image, off, [len(m) for m in members])
    try:
        return blob.download().tobytes(), blob.nbytes
    finally:
        blob.free()


def test_every_valid_case_alone_equals_zlib(gpu_ctx, valid):
    names = {n for n, _, _ in valid}
    assert {"empty", "stored_65280", "stored_len0_sync_flush", "fixed_256_literals", "fixed_len3_len258", "fixed_dist1_len258", "fixed_source_first_byte", "fixed_dist32768",
            "dynamic_level1", "dynamic_level6", "dynamic_level9", "huffman_only", "rle", "one_distinct_byte", "fibonacci_lengths_to_15", "repeat_codes_across_alphabets",
            "blocks_sync_and_full_flush"} <= names
    for name, member, want in valid:
        got, n = inflate(gpu_ctx, [member])
        assert n == len(want) and got == want, name
    t = gpu_ctx.timing()
    assert t["h2d_ms"] > 0 and t["pileup_ms"] > 0 and t["total_ms"] > 0


def test_the_cases_are_what_their_names_say(hip_lib):
    """the generator's side: zlib wrote what the case is meant to hold (block types by their headers, sizes at the BGZF maximum)"""
    assert "floria_hip_inflate_bgzf" in hip_lib.SYMBOLS                # the cases are for this entry point
    cases = {n: p for n, p, _, _ in ic.valid_cases()}
    assert len(EOF_MEMBER) == 28 and EOF_MEMBER[-4:] == b"\0\0\0\0"
    assert len(zlib.decompress(cases["stored_65280"], -15)) == ic.BGZF_MAX and cases["stored_65280"][0] & 7 == 0 and len(cases["stored_65280"]) > ic.BGZF_MAX + 5      # two stored blocks
    assert b"\x00\x00\xff\xff" in cases["stored_len0_sync_flush"]
    assert (cases["fixed_zlib"][0] >> 1) & 3 == 1 and (cases["dynamic_level6"][0] >> 1) & 3 == 2 and (cases["repeat_codes_across_alphabets"][0] >> 1) & 3 == 2
    assert len(zlib.decompress(cases["fixed_dist32768"], -15)) == ic.BGZF_MAX
    assert zlib.decompress(cases["repeat_codes_across_alphabets"], -15) == b"ABAABAAAA"
    assert b"\x00\x00\xff\xff" in cases["blocks_sync_and_full_flush"]


def test_eof_member_alone_and_between_others(gpu_ctx, valid):
    by = {n: (m, w) for n, m, w in valid}
    assert inflate(gpu_ctx, [EOF_MEMBER]) == (b"", 0)
    a, b = by["dynamic_level6"], by["fixed_len3_len258"]
    got, n = inflate(gpu_ctx, [a[0], EOF_MEMBER, b[0], EOF_MEMBER])
    assert got == a[1] + b[1] and n == len(a[1]) + len(b[1])
    assert inflate(gpu_ctx, []) == (b"", 0)


def test_odd_sizes_in_one_call_leave_no_output_offset_aligned(gpu_ctx, valid):
    by = {n: (m, w) for n, m, w in valid}
    order = ["one_byte", "empty", "stored_65280", "one_byte", "dynamic_level9", "one_byte", "empty", "three_bytes", "three_bytes"]
    offs = np.cumsum([len(by[n][1]) for n in order])
    assert {len(by[n][1]) for n in order} == {0, 1, 3, 65280} and all(o % 4 for o in offs)
    got, _ = inflate(gpu_ctx, [by[n][0] for n in order])
    assert got == b"".join(by[n][1] for n in order)


def test_more_members_than_the_grid_holds(gpu_ctx, valid):
    members = [m for _, m, _ in valid[2:12]]
    want = b"".join(w for _, _, w in valid[2:12])
    assert len(members) == 10
    gpu_ctx.set_option("inflate_slots", 3)
    try:
        got, _ = inflate(gpu_ctx, members)
    finally:
        gpu_ctx.set_option("inflate_slots", 0)
    assert got == want
    assert inflate(gpu_ctx, members)[0] == want
    # every valid case in one call, in an order other than the file's: the blob follows the member list
    image = b"".join(m for _, m, _ in valid)
    off = np.cumsum([0] + [len(m) for _, m, _ in valid[:-1]]).astype(np.uint64)
    ln = np.array([len(m) for _, m, _ in valid], np.uint32)
    perm = np.random.default_rng(2).permutation(len(valid))
    blob = gpu_ctx.inflate_bgzf(image, off[perm], ln[perm])
    assert blob.download().tobytes() == b"".join(valid[i][2] for i in perm)
    assert blob.download(5, 7).tobytes() == b"".join(valid[i][2] for i in perm)[5:12]
    blob.free()


def test_an_extra_subfield_before_bc(gpu_ctx):
    p = ic.deflate(ic.record_bytes(3000), 6)
    member = ic.bgzf_member(p, extra=b"XY" + struct.pack("<H", 5) + b"hello")
    assert inflate(gpu_ctx, [member])[0] == zlib.decompress(p, -15)


def test_malformed_members_are_refused_with_member_and_reason(gpu_ctx, hip_lib, valid):
    good = [valid[9][1], valid[5][1]]
    want = valid[9][2] + valid[5][2]
    reasons = {v: k for k, v in ic.STATUS.items()}
    bad = [(name, ic.bgzf_member(p, data=b"", isize=isize, crc=0), reasons[st]) for name, p, isize, st in ic.malformed_cases()]
    assert {r for _, _, r in bad} == {"bits ran out", "reserved block type", "LEN/NLEN mismatch", "over-subscribed code lengths", "distance beyond the bytes produced",
                                     "output longer than ISIZE", "output shorter than ISIZE"}
    p = ic.deflate(ic.record_bytes(3000), 6)
    data = zlib.decompress(p, -15)
    bad.append(("crc_bit", ic.bgzf_member(p, crc=(zlib.crc32(data) & 0xffffffff) ^ (1 << 13)), "CRC mismatch"))
    for name, member, reason in bad:
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            inflate(gpu_ctx, [good[0], member, good[1]])
        assert ei.value.code == -1 and "member 1:" in str(ei.value) and reason in str(ei.value), (name, str(ei.value))
        assert inflate(gpu_ctx, good)[0] == want, name                       # the context still serves a good call


def test_header_refusals_of_the_host_part(gpu_ctx, hip_lib):
    p = ic.deflate(b"floria" * 100, 6)
    good = ic.bgzf_member(p)

    def refused(code, word, members, n_bytes=None, lengths=None):
        image = b"".join(members)
        off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.inflate_bgzf(image[:n_bytes], off, lengths or [len(m) for m in members])
        assert ei.value.code == code and word in str(ei.value) and "member 1" in str(ei.value), str(ei.value)
        assert inflate(gpu_ctx, [good])[0] == b"floria" * 100
    refused(-1, "magic", [good, ic.bgzf_member(p, magic=b"\x1f\x8c\x08\x04")])
    refused(-1, "BC", [good, ic.bgzf_member(p, bc=b"BD")])
    refused(-1, "BSIZE", [good, ic.bgzf_member(p, bsize=len(good) + 1)])
    refused(-1, "n_bytes", [good, good], n_bytes=2 * len(good) - 1)
    refused(-4, "ISIZE", [good, ic.bgzf_member(p, isize=65537)])
    refused(-1, "method", [good, ic.bgzf_member(p, magic=b"\x1f\x8b\x07\x04")])


def test_the_bgzf_of_a_synth_bam_file(gpu_ctx, tmp_path):
    rng = np.random.default_rng(8)
    recs, pos = [], 100
    for i in range(400):
        n = int(rng.integers(100, 2500))
        pos += int(rng.integers(1, 200))
        recs.append(synth_bam.bam_record(0, pos, f"r{i}", 0, 60, [("M", n)], bytes(synth_bam.BASES[rng.integers(0, 4, size=n)]), rng.integers(5, 41, size=n).astype(np.uint8)))
    path = str(tmp_path / "s.bam")
    synth_bam.write_bam(path, [("c", 200000)], recs, block_bytes=30011)
    packed = open(path, "rb").read()
    members, raw = synth_bam._bgzf_members(packed)
    assert len(members) > 10
    off = np.array([m[0] for m in members], np.uint64)
    ln = np.diff(np.append(off, len(packed))).astype(np.uint32)
    blob = gpu_ctx.inflate_bgzf(packed, off, ln)
    assert blob.nbytes == len(raw) and blob.download().tobytes() == raw
    blob.free()
