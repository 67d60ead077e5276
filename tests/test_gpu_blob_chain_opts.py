"""`-m gpu`: floria_hip_blob_records_opt (csrc/inflate_kernel.h: blob_chain_kernel with FLORIA_CHAIN_CUT_TAIL / FLORIA_CHAIN_ONE_REF) against a plain walk of the
downloaded bytes: where every chain stops, why, and that the FILL pass lands where the COUNT pass said.  The parse model and the blob helper are those of
tests/test_gpu_blob_records.py."""
import ctypes as C
import struct

import numpy as np
import pytest

from floria_amd import _capi as capi
from floria_amd import synth_bam
from tests.test_gpu_blob_records import FIELDS, parse, to_blob

pytestmark = pytest.mark.gpu

CUT, ONE = capi.FLORIA_CHAIN_CUT_TAIL, capi.FLORIA_CHAIN_ONE_REF


def recs_of(tids, seed=9, lo=100, hi=400):
    """one record per entry of tids, l_seq in [lo, hi): a body of more than 32 + 50 bytes behind the prefix"""
    rng = np.random.default_rng(seed)
    out = []
    for i, tid in enumerate(tids):
        ln = int(rng.integers(lo, hi))
        out.append(synth_bam.bam_record(int(tid), 100 + 17 * i, f"r{i}", int(rng.integers(0, 4096)), int(rng.integers(0, 61)), [("M", ln)],
                                        bytes(synth_bam.BASES[rng.integers(0, 4, size=ln)]), rng.integers(5, 41, size=ln).astype(np.uint8)))
    return out, np.cumsum([0] + [len(r) for r in out]).astype(np.int64)


def model_stops(raw, begin, end, flags):
    """the two rules, on the host: (stop, why) of every chain"""
    stops, whys = [], []
    for b, e in zip(begin, end):
        o, n, ref0, why = int(b), 0, None, 0
        while o < e:
            if e - o < 4:
                why = 1; break
            bs, = struct.unpack_from("<I", raw, o)
            assert bs >= 32
            if bs > e - o - 4:
                why = 1; break
            if flags & ONE:
                ref, = struct.unpack_from("<i", raw, o + 4)
                if n == 0:
                    ref0 = ref
                elif ref != ref0:
                    why = 2; break
            n += 1; o += 4 + bs
        assert why != 1 or flags & CUT, "the model meets a cut tail without the flag"
        stops.append(o); whys.append(why)
    return stops, whys


def check(ctx, blob, raw, begin, end, flags):
    got = ctx.blob_records(blob, begin, end, flags=flags)
    stops, whys = model_stops(raw, begin, end, flags)
    cols, names, rec_off, stop = parse(raw, begin, stops)
    assert got["chain_stop"].tolist() == stops == stop and got["chain_why"].tolist() == whys and got["chain_rec_off"].tolist() == rec_off
    for f in FIELDS:
        assert got[f].tolist() == cols[f], f
    no = got["name_off"]
    assert [got["names"][int(no[i]):int(no[i + 1])].tobytes() for i in range(len(names))] == names
    return got


def test_flags_0_is_blob_records_field_for_field(gpu_ctx, hip_lib):
    recs, cuts = recs_of([0, 0, 1] * 14)
    raw = b"".join(recs)
    begin, end = [0, int(cuts[5]), int(cuts[20])], [int(cuts[5]), int(cuts[20]), int(cuts[42])]
    blob = to_blob(gpu_ctx, raw)
    try:
        old = gpu_ctx.blob_records(blob, begin, end)
        b, e = np.asarray(begin, np.uint64), np.asarray(end, np.uint64)
        out = C.POINTER(capi.CBlobRecords)()
        rc = hip_lib.load().floria_hip_blob_records_opt(gpu_ctx._h, blob._h, capi.ptr(b, C.c_uint64), capi.ptr(e, C.c_uint64), C.c_uint32(3), C.c_uint32(0), C.byref(out))
        assert rc == 0
        new = gpu_ctx._blob_records_result(out)
        # without a flag a cut record is the error it was
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.blob_records(blob, [0], [int(cuts[5]) - 1])
        assert ei.value.code == -1 and "chain 0 " in str(ei.value) and f"offset {int(cuts[4])}:" in str(ei.value) and "runs past" in str(ei.value)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.blob_records(blob, [0], [int(cuts[5])], flags=4)
        assert ei.value.code == -1 and "flags" in str(ei.value)
    finally:
        blob.free()
    assert sorted(old) == sorted(new) and len(old["offset"]) == 42
    for k in old:
        assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
    assert old["chain_why"].tolist() == [0, 0, 0] and old["chain_stop"].tolist() == end


def test_cut_tail_inside_the_prefix_the_fixed_bytes_the_body_and_behind_a_record(gpu_ctx):
    recs, cuts = recs_of([0] * 6)
    raw = b"".join(recs)
    at = int(cuts[3])
    assert len(recs[3]) > 4 + 32 + 50
    ends = [at + 1, at + 2, at + 3, at + 4 + 10, at + 4 + 32 + 50, int(cuts[4]) - 1, int(cuts[4]), at]
    blob = to_blob(gpu_ctx, raw)
    try:
        for flags in (CUT, CUT | ONE):
            got = check(gpu_ctx, blob, raw, [0] * len(ends), ends, flags)                 # the eight chains in one call
            assert got["chain_why"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
            assert got["chain_stop"].tolist() == [at] * 6 + [int(cuts[4]), at]
            assert np.diff(got["chain_rec_off"].astype(np.int64)).tolist() == [3] * 6 + [4, 3]
            for e in ends:                                                                # ... and each alone
                check(gpu_ctx, blob, raw, [0], [e], flags)
        got = check(gpu_ctx, blob, raw, [at], [at + 2], CUT)                              # a chain that is nothing but a cut prefix
        assert got["chain_why"].tolist() == [1] and len(got["offset"]) == 0
    finally:
        blob.free()


def test_one_ref_stops_in_front_of_the_first_record_of_another_reference(gpu_ctx, hip_lib):
    tids = [0, 0, 1] + [0, 1] + [5] + [3, 3, 3, 3] + [-1, -1, 2]
    recs, cuts = recs_of(tids)
    raw = b"".join(recs)
    bounds = [0, 3, 5, 6, 10, 13]
    begin, end = [int(cuts[i]) for i in bounds[:-1]], [int(cuts[i]) for i in bounds[1:]]
    blob = to_blob(gpu_ctx, raw)
    try:
        for flags in (ONE, ONE | CUT):
            got = check(gpu_ctx, blob, raw, begin, end, flags)
            assert got["chain_why"].tolist() == [2, 2, 0, 0, 2]
            assert got["chain_stop"].tolist() == [int(cuts[2]), int(cuts[4]), int(cuts[6]), int(cuts[10]), int(cuts[12])]
            assert np.diff(got["chain_rec_off"].astype(np.int64)).tolist() == [2, 1, 1, 4, 2]
        # ONE_REF alone does not forgive a cut record
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.blob_records(blob, [int(cuts[6])], [int(cuts[9]) - 5], flags=ONE)
        assert ei.value.code == -1 and "chain 0 " in str(ei.value) and f"offset {int(cuts[8])}:" in str(ei.value) and "runs past" in str(ei.value)
    finally:
        blob.free()


def test_both_flags_whichever_comes_first(gpu_ctx):
    recs, cuts = recs_of([0, 0, 1, 1] + [0, 0, 0, 1] + [0, 0, 1])
    raw = b"".join(recs)
    begin = [0, int(cuts[4]), int(cuts[8])]
    end = [int(cuts[4]) - 7,          # the other reference (record 2) stands before the cut (in record 3)
           int(cuts[7]) - 7,          # the cut (in record 6) stands before the other reference (record 7)
           int(cuts[11]) - 7]         # the cut record is itself of another reference: its refID is not read, a cut tail
    blob = to_blob(gpu_ctx, raw)
    try:
        got = check(gpu_ctx, blob, raw, begin, end, CUT | ONE)
        assert got["chain_why"].tolist() == [2, 1, 1]
        assert got["chain_stop"].tolist() == [int(cuts[2]), int(cuts[6]), int(cuts[10])]
    finally:
        blob.free()


def test_block_size_31_is_refused_with_chain_and_offset_under_both_flags(gpu_ctx, hip_lib):
    recs, cuts = recs_of([0] * 12)
    short = bytearray(b"".join(recs))
    short[int(cuts[8]):int(cuts[8]) + 4] = struct.pack("<I", 31)
    blob = to_blob(gpu_ctx, bytes(short))
    try:
        for flags in (CUT, ONE, CUT | ONE):
            with pytest.raises(hip_lib.FloriaHipError) as ei:
                gpu_ctx.blob_records(blob, [0, int(cuts[5])], [int(cuts[5]), len(short)], flags=flags)
            assert ei.value.code == -1 and "chain 1 " in str(ei.value) and f"offset {int(cuts[8])}:" in str(ei.value) and "block_size below" in str(ei.value), str(ei.value)
        good = gpu_ctx.blob_records(blob, [0], [int(cuts[8]) + 3], flags=CUT)             # the context and the blob still serve a good call
        assert len(good["offset"]) == 8 and good["chain_why"].tolist() == [1]
    finally:
        blob.free()


def test_300_chains_of_different_lengths_fill_lands_where_count_said(gpu_ctx):
    """more chains than one 256-thread workgroup of the chain kernel: chain c has c % 7 + 1 records; every fourth ends in a record of another reference, every
    fourth (the next) has its end cut 1 .. 30 bytes into its last record"""
    n_rec = [c % 7 + 1 for c in range(300)]
    tids = []
    for c, n in enumerate(n_rec):
        t = [c % 3] * n
        if c % 4 == 0 and n > 1:
            t[-1] = 7
        tids += t
    recs, cuts = recs_of(tids, lo=1, hi=60)
    raw = b"".join(recs)
    first = np.cumsum([0] + n_rec)
    begin = [int(cuts[first[c]]) for c in range(300)]
    end = [int(cuts[first[c + 1]]) - (c % 30 + 1 if c % 4 == 1 else 0) for c in range(300)]
    blob = to_blob(gpu_ctx, raw)
    try:
        got = check(gpu_ctx, blob, raw, begin, end, CUT | ONE)
    finally:
        blob.free()
    want = [n - 1 if (c % 4 == 0 and n > 1) or c % 4 == 1 else n for c, n in enumerate(n_rec)]
    assert np.diff(got["chain_rec_off"].astype(np.int64)).tolist() == want
    assert sorted(set(got["chain_why"].tolist())) == [0, 1, 2]
    # FILL: record k of chain c is the k-th record behind begin[c]
    assert got["offset"].tolist() == [int(cuts[first[c] + k]) for c in range(300) for k in range(want[c])]
