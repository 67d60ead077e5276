"""`-m gpu`: floria_hip_blob_sequences (csrc/blob_seq_kernel.h) against the numpy model of tests/blob_seq_model.py: the letters and qualities frag_sequences
(host/ingest.cpp) makes of a record, for records that lie at any offset of a blob."""
import ctypes as C

import numpy as np
import pytest

from floria_amd import _capi as capi
from tests import blob_seq_model as model
from tests.test_gpu_blob_records import to_blob

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)


def lay_out(parts, first=0, gaps=None, seed=2):
    """parts: (packed bytes, quality bytes) per record -> raw bytes with every range somewhere behind `first` bytes of filler, gaps[i] bytes of filler in front of
    record i's sequence and gaps[i] + 1 between it and its qualities; (raw, seq_off, l_seq, qual_off)"""
    rng = np.random.default_rng(seed)
    fill = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    raw, seq_off, l_seq, qual_off = bytearray(fill(first)), [], [], []
    for i, (packed, qual) in enumerate(parts):
        g = 0 if gaps is None else int(gaps[i])
        raw += fill(g); seq_off.append(len(raw)); raw += bytes(packed)
        raw += fill(g + 1); qual_off.append(len(raw)); raw += bytes(qual)
        l_seq.append(len(qual))
        assert len(packed) == (len(qual) + 1) // 2
    raw += fill(3)
    return bytes(raw), seq_off, l_seq, qual_off


def random_parts(lengths, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, size=(n + 1) // 2, dtype=np.uint8), rng.integers(0, 256, size=n, dtype=np.uint8)) for n in lengths]


def check(ctx, raw, seq_off, l_seq, qual_off):
    blob = to_blob(ctx, raw)
    try:
        assert blob.download().tobytes() == raw
        base_off, bases, quals = ctx.blob_sequences(blob, seq_off, l_seq, qual_off)
    finally:
        blob.free()
    w_off, w_bases, w_quals = model.sequences(raw, seq_off, l_seq, qual_off)
    assert base_off.dtype == np.uint64 and np.array_equal(base_off, w_off)
    assert bases.dtype == np.uint8 and len(bases) == int(w_off[-1]) and np.array_equal(bases, w_bases)
    assert quals.dtype == np.uint8 and len(quals) == int(w_off[-1]) and np.array_equal(quals, w_quals)
    return base_off, bases, quals


@pytest.mark.parametrize("first", [0, 1])
def test_every_length_at_odd_and_even_offsets(gpu_ctx, first):
    """each length alone (its output starts on an 8-byte boundary) and all of them in one call (every output alignment), the ranges at odd and at even offsets:
    `first` shifts them all by one, and the gap of i % 2 bytes changes the parity from record to record"""
    parts = random_parts(LENGTHS, seed=3)
    for p in parts:
        check(gpu_ctx, *lay_out([p], first=first))
    raw, so, ls, qo = lay_out(parts, first=first, gaps=[i % 2 for i in range(len(parts))])
    assert {o % 2 for o in so} == {0, 1} and {o % 2 for o in qo} == {0, 1}
    check(gpu_ctx, raw, so, ls, qo)
    check(gpu_ctx, raw, so[::-1], ls[::-1], qo[::-1])                     # the same records in another order: other output alignments
    assert gpu_ctx.timing()["pileup_ms"] > 0
    base_off, bases, quals = check(gpu_ctx, raw, [], [], [])              # no record at all
    assert base_off.tolist() == [0] and len(bases) == 0 and len(quals) == 0
    base_off, bases, quals = check(gpu_ctx, raw, [len(raw), 0], [0, 0], [0, len(raw)])      # nothing but empty records, at the blob's two ends
    assert base_off.tolist() == [0, 0, 0]


def test_all_16_codes_in_both_nibbles_and_the_padding_of_an_odd_length(gpu_ctx):
    packed = np.arange(256, dtype=np.uint8)                               # every pair of codes
    qual = np.full(512, 30, np.uint8)
    for first in (0, 1, 2, 3):                                            # the groups begin on a high nibble (even) and on a low one (odd)
        lead = (np.full((first + 1) // 2, 0x48, np.uint8), np.full(first, 7, np.uint8))
        parts = [lead, (packed, qual)] if first else [(packed, qual)]
        base_off, bases, _ = check(gpu_ctx, *lay_out(parts))
        got = bases[int(base_off[-2]):].reshape(256, 2)
        letter = {1: "A", 2: "C", 4: "G", 8: "T"}
        for b in range(256):
            assert bytes(got[b]).decode() == letter.get(b >> 4, "A") + letter.get(b & 15, "A"), b
    # odd lengths whose padding nibble holds a code: C (2), T (8), N (15) must not appear; the next record's first letter stands right behind
    parts = [(np.array([0x12], np.uint8), [1]), (np.array([0x48, 0x18], np.uint8), [2, 3, 4]), (np.array([0x8f], np.uint8), [5]), (np.array([0x21], np.uint8), [6, 7])]
    _, bases, quals = check(gpu_ctx, *lay_out(parts))
    assert bytes(bases).decode() == "A" + "GTA" + "T" + "CA" and quals.tolist() == [34, 35, 36, 37, 38, 39, 40]


def test_qualities_0_222_223_254_255(gpu_ctx):
    q = np.array([0, 222, 223, 254, 255] * 5 + [0], np.uint8)             # 26 bytes: head, whole groups and tail of the output all see the rule
    packed = np.full(13, 0x11, np.uint8)
    _, _, quals = check(gpu_ctx, *lay_out([(packed[:1], q[:1]), (packed, q)]))
    assert quals.tolist() == [33] + [33, 255, 255, 255, 255] * 5 + [33]


def test_2000_random_records_of_mixed_lengths(gpu_ctx):
    """more records than one pass of the grid's wavefronts needs no more than this; every output range is bordered by its neighbours', so the equality with the
    model says that no record wrote outside its own.  What is NOT observed: the device buffers' slack behind the last record's range (the call returns exactly
    `total` bytes of each array; a write past it on the device would go unseen here - the kernel's `k < len` guard is what rules it out)."""
    rng = np.random.default_rng(11)
    lengths = np.where(rng.random(2000) < 0.1, rng.integers(0, 9, size=2000), rng.integers(0, 700, size=2000))
    lengths[:4] = [0, 0, 1, 1025]
    parts = random_parts(lengths.tolist(), seed=12)
    raw, so, ls, qo = lay_out(parts, first=1, gaps=rng.integers(0, 4, size=2000))
    order = rng.permutation(2000)                                         # the output order is the call's, not the blob's
    take = lambda a: [a[i] for i in order]
    base_off, _, _ = check(gpu_ctx, raw, take(so), take(ls), take(qo))
    assert len({int(o) % 8 for o in base_off}) == 8


def test_every_refusal(gpu_ctx, hip_lib):
    parts = random_parts([9, 10], seed=5)
    raw, so, ls, qo = lay_out(parts)
    blob = to_blob(gpu_ctx, raw)
    n = len(raw)
    try:
        for s, l, q, what, rec in (([so[0], n - 4], [9, 10], qo, "sequence", 1),       # 5 packed bytes from n - 4
                                   ([n + 1, so[1]], [0, 10], qo, "sequence", 0),       # an empty range behind the blob's end
                                   (so, [9, 10], [qo[0], n - 9], "quality", 1),
                                   ([so[0]], [2 ** 32 - 1], [qo[0]], "sequence", 0)):
            with pytest.raises(hip_lib.FloriaHipError) as ei:
                gpu_ctx.blob_sequences(blob, s, l, q)
            assert ei.value.code == -1 and f"the {what} bytes of record {rec} " in str(ei.value), str(ei.value)
        other = hip_lib.FloriaHip(0)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            other.blob_sequences(blob, so, ls, qo)
        assert ei.value.code == -1 and "another context" in str(ei.value)
        other.close()
        # null arguments
        L = hip_lib.load()
        a_so, a_ls, a_qo = np.asarray(so, np.uint64), np.asarray(ls, np.uint32), np.asarray(qo, np.uint64)
        out = C.POINTER(capi.CBlobSequences)()
        p = lambda a, t: capi.ptr(a, t)
        good = (gpu_ctx._h, blob._h, p(a_so, C.c_uint64), p(a_ls, C.c_uint32), p(a_qo, C.c_uint64), C.c_uint64(2), C.byref(out))
        for k in (0, 1, 2, 3, 4, 6):
            args = list(good)
            args[k] = None
            assert L.floria_hip_blob_sequences(*args) == -1 and b"null argument" in L.floria_hip_last_error(), k
        L.floria_hip_blob_sequences_free(None)
        # the context and the blob still serve a good call
        w = model.sequences(raw, so, ls, qo)
        got = gpu_ctx.blob_sequences(blob, so, ls, qo)
        assert all(np.array_equal(a, b) for a, b in zip(got, w))
    finally:
        blob.free()
