"""`-m gpu`: floria_hip_blob_estimate (csrc/estimate_kernel.h) against the column model of tests/estimate_model.py: every sampled column (group, position, total,
most), every record's hits, the state carried out and `done`, on hand-built records laid into a blob at arbitrary offsets."""
import ctypes as C
import struct

import numpy as np
import pytest

from floria_amd import _capi as capi
from tests import estimate_model as model
from tests.test_gpu_blob_records import to_blob

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)


def rec(pos, cigar, codes=None, l_seq=None, seed=0, cg=False):
    """a record of the model, its codes random unless given; l_seq defaults to what the CIGAR consumes.  cg: laid out as a CG record (lay_out)"""
    cigar = [(int(op), int(ln)) for op, ln in cigar]
    if codes is None:
        n = sum(ln for op, ln in cigar if op in model.QUERY_OPS) if l_seq is None else l_seq
        codes = np.random.default_rng([seed, pos, len(cigar)]).integers(0, 16, size=n)
    r = (int(pos), cigar, np.asarray(codes, np.int64))
    return r + ("cg",) if cg else r


def pack(codes):
    c = np.concatenate([np.asarray(codes, np.uint8), np.zeros(len(codes) & 1, np.uint8)])
    return (c[0::2] << 4 | c[1::2]).astype(np.uint8).tobytes()


def lay_out(groups, seed=1):
    """the records' CIGAR words and packed bases somewhere in a byte string, filler of 0 .. 3 bytes around them (every alignment); a CG record is a whole BAM record
    with the kSmN placeholder whose real CIGAR stands in a CG:B,I array behind its qualities -> (raw, dict of the call's arrays)"""
    rng = np.random.default_rng(seed)
    fill = lambda: rng.integers(0, 256, size=int(rng.integers(0, 4)), dtype=np.uint8).tobytes()
    raw = bytearray(fill())
    a = dict(pos=[], cigar_off=[], n_cigar=[], seq_off=[], l_seq=[], group_off=[0])
    for g in groups:
        for r in g:
            pos, cigar, codes = r[:3]
            words = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar)
            if len(r) == 4:
                l_seq = len(codes)
                body = struct.pack("<iiBBHHHIiii", 0, pos, 2, 60, 0, 2, 0, l_seq, -1, -1, 0) + b"r\0" + struct.pack("<II", l_seq << 4 | S, model.span_end(pos, cigar) - pos << 4 | N)
                raw += struct.pack("<I", len(body) + (l_seq + 1) // 2 + l_seq + 8 + len(words))
                raw += body
                a["seq_off"].append(len(raw)); raw += pack(codes) + bytes(l_seq)
                raw += b"CGBI" + struct.pack("<I", len(cigar))
                a["cigar_off"].append(len(raw)); raw += words
            else:
                raw += fill(); a["cigar_off"].append(len(raw)); raw += words
                raw += fill(); a["seq_off"].append(len(raw)); raw += pack(codes)
            a["pos"].append(pos); a["n_cigar"].append(len(cigar)); a["l_seq"].append(len(codes))
        a["group_off"].append(len(a["pos"]))
    raw += fill() + b"\0"
    return bytes(raw), a


def compare(got, want, what=""):
    cols = want["cols"]
    for k, f in enumerate(("col_group", "col_pos", "col_total", "col_most")):
        assert got[f].tolist() == [c[k] for c in cols], (what, f)
    assert got["rec_hits"].tolist() == want["rec_hits"].tolist(), what
    assert (got["count"], got["n_err"], got["done"]) == (want["count"], want["n_err"], want["done"]), what


def check(ctx, groups, stop, count=0, n_err=0, window=0, blob=None, arrays=None):
    want = model.estimate([[r[:3] for r in g] for g in groups], stop, count, n_err)
    own = blob is None
    if own:
        raw, arrays = lay_out(groups)
        blob = to_blob(ctx, raw)
    ctx.set_option("estimate_window", window)
    try:
        got = ctx.blob_estimate(blob, stop=stop, count=count, n_err=n_err, **arrays)
    finally:
        ctx.set_option("estimate_window", 0)
        if own:
            blob.free()
    compare(got, want, (stop, count, n_err, window))
    return got, want


def by_pos(g):
    return sorted(g, key=lambda r: r[0])


def pile(n, pos, length, seed=0):
    return [rec(pos, [(M, length)], seed=seed + i) for i in range(n)]


def test_a_column_of_four_then_five_and_a_shallow_run_longer_than_a_wavefront(gpu_ctx):
    g = by_pos(pile(4, 100, 3500) + [rec(101, [(M, 3500)], seed=9)])
    got, want = check(gpu_ctx, [g], stop=4)
    assert want["cols"][0][1:3] == (100, 4) and want["cols"][1][1:3] == (101, 5) and want["n_err"] == 4 and want["done"]
    assert gpu_ctx.timing()["pileup_ms"] > 0 and gpu_ctx.timing()["d2h_ms"] > 0
    g = by_pos(pile(4, 100, 3500) + [rec(170, [(M, 3500)], seed=9)])
    got, want = check(gpu_ctx, [g], stop=3)
    assert [c[2] for c in want["cols"][:71]] == [4] * 70 + [5] and want["cols"][70][1] == 170
    got, want = check(gpu_ctx, [pile(4, 7, 300)], stop=3)                 # never deep: every column is sampled and count does not move
    assert len(want["cols"]) == 300 and want["count"] == 0 and want["n_err"] == 0 and not want["done"]


def test_cigar_operations_at_and_before_a_sampled_column(gpu_ctx):
    base = pile(4, 0, 2600)
    g = base + [rec(0, [(M, 10), (D, 5), (M, 2590)], seed=20), rec(0, [(M, 10), (N, 5), (EQ, 2590)], seed=21)]
    for count in (988, 990, 985):                                         # the sampled column inside, at the first position of, and at the last before the deletion / refskip
        got, want = check(gpu_ctx, [g], stop=3, count=count)
    assert want["cols"][0][1:3] == (15, 6)
    got, want = check(gpu_ctx, [g], stop=3, count=988)
    assert [c[1:3] for c in want["cols"][:4]] == [(12, 4), (13, 4), (14, 4), (15, 6)]
    g = base + [rec(0, [(H, 5), (S, 3), (M, 4), (I, 2), (P, 1), (M, 6), (X, 3), (EQ, 2600)], seed=22),
                rec(2, [(S, 7), (EQ, 3), (I, 1), (X, 5), (D, 2), (M, 2600), (S, 4), (H, 9)], seed=23)]
    for count in (0, 995, 993, 989, 985, 1):
        check(gpu_ctx, [g], stop=5, count=count)


def test_all_16_codes_in_both_nibbles(gpu_ctx):
    """four records, so every column is sampled (and discarded): each column's total and most are in the result"""
    codes = [np.arange(64) % 16, (np.arange(64) // 2) % 16, (np.arange(64) * 7 + 1) % 16, np.arange(64)[::-1] % 16]
    g = [rec(0, [(M, 64)], codes=c) for c in codes] + [rec(65, [(S, 1), (M, 63)], codes=c) for c in codes]
    got, want = check(gpu_ctx, [g], stop=3)
    assert len(want["cols"]) == 127 and {c[3] for c in want["cols"]} >= {1, 2}
    seen = {(int(c[p]), p & 1) for c in codes for p in range(64)}
    assert len(seen) == 32


def test_degenerate_records(gpu_ctx):
    g = pile(3, 0, 40) + [rec(0, [(M, 40)], l_seq=0), rec(5, [(S, 5)], seed=1), rec(6, [(I, 3), (H, 2)], seed=2), rec(20, [(M, 50)], l_seq=20, seed=3), rec(60, [(M, 30)], l_seq=7, seed=4),
                          rec(95, [(P, 3)], l_seq=0)]
    got, want = check(gpu_ctx, [g], stop=3)
    cols = {c[1]: c[2] for c in want["cols"]}
    assert cols[0] == 3 and cols[39] == 4 and cols[40] == 0 and cols[66] == 1 and cols[69] == 0 and cols[89] == 0 and cols[95] == 0 and 90 not in cols
    assert want["rec_hits"].tolist()[3:] == [0, 0, 0, 20, 7, 0]
    check(gpu_ctx, [pile(5, 0, 40) + g[3:]], stop=7, count=995)


def long_cigar(n_ops, seed):
    rng = np.random.default_rng(seed)
    ops = [(M, 2), (D, 1), (EQ, 1), (I, 2), (X, 3), (N, 2), (M, 1), (S, 0), (P, 1)]
    return [ops[k % len(ops)] if k % 11 else (M, int(rng.integers(1, 5))) for k in range(n_ops)]


@pytest.mark.parametrize("n_ops", [1, 64, 65, 5000])
def test_cigars_of_1_64_65_and_5000_operations(gpu_ctx, n_ops):
    """a depth of four samples every column, so every operation of the long CIGAR is asked for a base; a fifth record makes some columns deep"""
    cig = long_cigar(n_ops, 5) if n_ops > 1 else [(M, 90)]
    g = [rec(0, cig, seed=s) for s in range(3)] + [rec(0, cig, seed=3, l_seq=max(1, sum(ln for op, ln in cig if op in model.QUERY_OPS) - 9))]
    check(gpu_ctx, [g], stop=3)
    span = model.span_end(0, cig)
    check(gpu_ctx, [by_pos(g + [rec(span // 2, [(M, span)], seed=8)])], stop=5, window=1024)
    check(gpu_ctx, [g + [rec(0, cig, seed=9), rec(0, cig, seed=10, cg=True)]], stop=7, count=700)      # deep everywhere: one column per 1000, far into the CIGAR


def test_a_cg_record_whose_cigar_stands_in_its_aux_bytes(gpu_ctx):
    cig = [(S, 3), (M, 700), (D, 4), (M, 700), (I, 2), (M, 900)]
    g = [rec(10, cig, seed=s, cg=True) for s in range(5)] + [rec(10, cig, seed=6)]
    raw, a = lay_out([g])
    assert raw[a["cigar_off"][0] - 8:a["cigar_off"][0] - 4] == b"CGBI" and a["cigar_off"][0] > a["seq_off"][0]
    check(gpu_ctx, [g], stop=3)
    check(gpu_ctx, [g], stop=3, count=999)


def two_groups():
    g0 = by_pos(pile(5, 0, 1500) + pile(5, 4000, 1200, seed=30) + [rec(4100, [(M, 50), (N, 900), (M, 100)], seed=31)])      # positions 1500 .. 3999 are not covered
    g1 = by_pos(pile(6, 50_000, 2500, seed=40) + pile(2, 50_700, 600, seed=41))
    return [g0, [], g1]


@pytest.mark.parametrize("count", [0, 999, 1000])
def test_two_groups_a_gap_and_the_count_carried_in(gpu_ctx, count):
    got, want = check(gpu_ctx, two_groups(), stop=7, count=count)
    assert {c[0] for c in want["cols"]} == {0, 2} and not any(1500 <= c[1] < 4000 for c in want["cols"])
    check(gpu_ctx, two_groups(), stop=7, count=count, n_err=4)
    got, want = check(gpu_ctx, two_groups(), stop=7, count=count, n_err=7)      # already at stop: nothing is sampled
    assert want["done"] and not want["cols"] and got["count"] == count


def test_one_call_equals_two_calls_with_the_state_carried(gpu_ctx):
    groups = two_groups()
    whole, _ = check(gpu_ctx, groups, stop=6, count=400)
    first, _ = check(gpu_ctx, groups[:1], stop=6, count=400)
    second, _ = check(gpu_ctx, groups[2:], stop=6, count=first["count"], n_err=first["n_err"])
    assert not first["done"] and second["done"] == whole["done"]
    assert (second["count"], second["n_err"]) == (whole["count"], whole["n_err"])
    for f in ("col_pos", "col_total", "col_most", "rec_hits"):
        assert np.concatenate([first[f], second[f]]).tolist() == whole[f].tolist(), f
    assert np.concatenate([first["col_group"], second["col_group"] + 2]).tolist() == whole["col_group"].tolist()


@pytest.mark.parametrize("window", [1024, 1000, 37])
def test_windows_change_nothing(gpu_ctx, window):
    groups = two_groups()
    for count in (0, 977):
        base, _ = check(gpu_ctx, groups, stop=7, count=count)
        cut, _ = check(gpu_ctx, groups, stop=7, count=count, window=window)
        assert all(np.array_equal(base[f], cut[f]) for f in ("col_group", "col_pos", "col_total", "col_most", "rec_hits"))
    # a shallow run over a window's edge (the windows begin at the group's first position, 1000): four records to 2100, a fifth from 2060
    g = by_pos(pile(4, 1000, 1100, seed=50) + [rec(2060, [(M, 2000)], seed=51)])
    got, want = check(gpu_ctx, [g], stop=3, count=980, window=window)
    assert [c[2] for c in want["cols"][:1041]] == [4] * 1040 + [5] and want["cols"][0][1] == 1020 and want["cols"][1040][1] == 2060
    # a record over three windows and more, its deletion and its insertion in different ones
    g = pile(5, 0, 900, seed=60) + [rec(3, [(M, 1000), (D, 30), (M, 1100), (I, 5), (M, 1200)], seed=61)] + pile(4, 2500, 700, seed=62)
    check(gpu_ctx, [g], stop=4, count=1, window=window)
    check(gpu_ctx, [g], stop=4, count=985, window=window)


def test_stop_1000_is_reached(gpu_ctx):
    """500 records of 10 kb at depth 5: about a million columns, one in a thousand sampled"""
    rng = np.random.default_rng(70)
    g = [rec(2000 * i, [(M, 10_000)], codes=np.where(rng.random(10_000) < 0.1, rng.integers(0, 16, size=10_000), 1 << (np.arange(10_000) + 2000 * i) % 4)) for i in range(504)]
    got, want = check(gpu_ctx, [g], stop=1000)
    assert want["done"] and want["n_err"] == 1000 and len({c[3] for c in want["cols"]}) > 1
    lengths = model.lengths_of([g], got["rec_hits"])
    assert lengths == [(10_000, int(got["col_total"].sum()))] and model.result(want["cols"], lengths)[0] == 10_000


def random_groups(rng):
    groups = []
    for _ in range(int(rng.integers(1, 4))):
        g = []
        for _ in range(int(rng.integers(0, 13))):
            cig = [(int(rng.choice([M, M, M, EQ, X, I, D, N, S, H, P])), int(rng.integers(0, 40))) for _ in range(int(rng.integers(1, 9)))]
            need = sum(ln for op, ln in cig if op in model.QUERY_OPS)
            l_seq = need if rng.random() < 0.7 else int(rng.integers(0, need + 5))
            g.append(rec(int(rng.integers(0, 300)), cig, l_seq=l_seq, seed=int(rng.integers(1 << 30))))
        groups.append(sorted(g, key=lambda r: r[0]))
    return groups


def test_300_random_record_sets(gpu_ctx):
    """all sets in one blob; every set with a random state carried in, stop and window"""
    rng = np.random.default_rng(80)
    sets = [random_groups(rng) for _ in range(300)]
    raw, arrays = bytearray(), []
    for k, groups in enumerate(sets):
        part, a = lay_out(groups, seed=k)
        a["cigar_off"] = [o + len(raw) for o in a["cigar_off"]]; a["seq_off"] = [o + len(raw) for o in a["seq_off"]]
        raw += part; arrays.append(a)
    blob = to_blob(gpu_ctx, bytes(raw))
    try:
        for groups, a in zip(sets, arrays):
            check(gpu_ctx, groups, stop=int(rng.integers(3, 8)), count=int(rng.integers(0, 2100)) if rng.random() < 0.5 else int(rng.choice([0, 1000, 999])), n_err=int(rng.integers(0, 3)),
                  window=int(rng.choice([0, 37, 256, 1024])), blob=blob, arrays=a)
    finally:
        blob.free()


def test_every_refusal_leaves_the_context_usable(gpu_ctx, hip_lib):
    groups = [pile(5, 10, 1200), pile(5, 40, 1200, seed=3)]
    raw, a = lay_out(groups)
    blob = to_blob(gpu_ctx, raw)
    n_bytes = len(raw)
    want = model.estimate(groups, 3)

    def good():
        compare(gpu_ctx.blob_estimate(blob, stop=3, **a), want)

    def change(**kw):
        b = {k: list(v) for k, v in a.items()}
        for k, (i, v) in kw.items():
            b[k][i] = v
        return b

    try:
        good()
        for arrays, code, text in ((change(cigar_off=(7, n_bytes - 3)), -1, "the CIGAR bytes of record 7 reach past the blob"),
                                   (change(cigar_off=(2, n_bytes + 1)), -1, "the CIGAR bytes of record 2 reach past the blob"),
                                   (change(n_cigar=(9, 2 ** 32 - 1)), -1, "the CIGAR bytes of record 9 reach past the blob"),
                                   (change(seq_off=(3, n_bytes - 10)), -1, "the sequence bytes of record 3 reach past the blob"),
                                   (change(l_seq=(0, 2 ** 32 - 1)), -1, "the sequence bytes of record 0 reach past the blob"),
                                   (change(n_cigar=(4, 0)), -1, "record 4 has no CIGAR operation"),
                                   (change(pos=(6, -1)), -1, "record 6 has a negative pos"),
                                   (change(pos=(8, 9)), -1, "record 8: pos descends inside group 1"),
                                   (change(group_off=(0, 1)), -1, "group_off does not start at 0"),
                                   (change(group_off=(1, 11)), -1, "group_off descends at group 1"),
                                   (change(group_off=(2, 9)), -1, "group_off ends at 9, not at the 10 records"),
                                   (change(pos=(9, 2 ** 31 - 1200)), -4, "record 9 ends at 2147483648, beyond 2^31 - 1")):
            with pytest.raises(hip_lib.FloriaHipError) as ei:
                gpu_ctx.blob_estimate(blob, stop=3, **arrays)
            assert ei.value.code == code and text in str(ei.value), (text, str(ei.value))
            good()
        assert a["pos"][5] == 40                                           # (pos may descend from one group to the next)
        other = hip_lib.FloriaHip(0)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            other.blob_estimate(blob, stop=3, **a)
        assert ei.value.code == -1 and "another context" in str(ei.value)
        other.close()
        good()
        L = hip_lib.load()
        keep = {k: np.ascontiguousarray(v, t) for (k, v), t in zip(a.items(), (np.int32, np.uint64, np.uint32, np.uint64, np.uint32, np.uint64))}
        fields = [capi.ptr(keep[k], t) for k, t in (("pos", C.c_int32), ("cigar_off", C.c_uint64), ("n_cigar", C.c_uint32), ("seq_off", C.c_uint64), ("l_seq", C.c_uint32))]
        recs = capi.CEstimateRecords(10, *fields, 2, capi.ptr(keep["group_off"], C.c_uint64))
        state = capi.CEstimateState(0, 0)
        out = C.POINTER(capi.CEstimateResult)()
        call = (gpu_ctx._h, blob._h, C.byref(recs), C.c_uint32(3), C.byref(state), C.byref(out))
        for k in (0, 1, 2, 4, 5):
            args = list(call)
            args[k] = None
            assert L.floria_hip_blob_estimate(*args) == -1 and b"null argument" in L.floria_hip_last_error(), k
        for f in ("pos", "cigar_off", "n_cigar", "seq_off", "l_seq", "group_off"):
            broken = capi.CEstimateRecords(10, *fields, 2, capi.ptr(keep["group_off"], C.c_uint64))
            setattr(broken, f, None)
            assert L.floria_hip_blob_estimate(gpu_ctx._h, blob._h, C.byref(broken), C.c_uint32(3), C.byref(state), C.byref(out)) == -1 and b"null argument" in L.floria_hip_last_error(), f
        L.floria_hip_estimate_result_free(None)
        with pytest.raises(hip_lib.FloriaHipError):
            gpu_ctx.set_option("estimate_window", -1)
        with pytest.raises(hip_lib.FloriaHipError):
            gpu_ctx.set_option("estimate_window", 2 ** 30 + 1)
        good()
    finally:
        blob.free()
