"""`-m gpu`: BAM file -> floria_hip_inflate_bgzf -> floria_hip_blob_records -> floria_hip_pileup_records_resident_blob -> floria_hip_assemble_contigs_opt, against the same
calls fed from a host blob: every summary field and every download field of every handle must be equal, with and without reference sequences and with one block walk.
No record byte goes up on the handle's path."""
import ctypes as C
import struct

import numpy as np
import pytest

from floria_amd import _capi as capi
from floria_amd import synth, synth_bam
from tests import pileup_model as pm
from tests import plan_model

pytestmark = pytest.mark.gpu

SUMMARY = ("cell_off", "first_snp", "last_snp", "ref_end")


def read_fasta(path):
    seqs, cur = {}, None
    for line in open(path):
        if line.startswith(">"):
            cur = line[1:].split()[0]; seqs[cur] = []
        else:
            seqs[cur].append(line.strip())
    return {k: "".join(v).encode() for k, v in seqs.items()}


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """name -> file prefix: the hand-built supplementary + paired set and the small noisy long-read set of tests/test_gpu_pileup.py"""
    from tests.test_gpu_pileup import hand_built
    d = tmp_path_factory.mktemp("blob")
    hand = str(d / "h")
    hand_built(hand)
    plan_model.add_case_records(hand)                           # the paired and supplementary cases of the fragment plan
    noisy = str(d / "n")
    synth_bam.write_dataset(noisy, [synth.make_config_contig(1, 1, 0.6, keep_layout=True)], seed=7, sub_rate=0.12)
    return dict(hand=hand, noisy=noisy)


class World:
    """one data set on the device: the blob, its record table, and the arguments of both pileup calls"""

    def __init__(self, ctx, prefix):
        packed = open(prefix + ".bam", "rb").read()
        members, raw = synth_bam._bgzf_members(packed)
        off = np.array([m[0] for m in members], np.uint64)
        self.raw = np.frombuffer(raw, np.uint8)
        self.blob = ctx.inflate_bgzf(packed, off, np.diff(np.append(off, len(packed))).astype(np.uint32))
        assert self.blob.nbytes == len(raw)
        # the BAM header is header-sized data the host reads itself: text, then the targets
        head = self.blob.download(0, min(len(raw), 1 << 16)).tobytes()
        assert head[:4] == b"BAM\1"
        o = 8 + struct.unpack_from("<I", head, 4)[0]
        n_ref, = struct.unpack_from("<I", head, o)
        o += 4
        names = []
        for _ in range(n_ref):
            ln, = struct.unpack_from("<I", head, o)
            names.append(head[o + 4:o + 4 + ln - 1].decode())
            o += 8 + ln
        self.table = t = ctx.blob_records(self.blob, [o], [len(raw)])
        assert int(t["chain_stop"][0]) == len(raw) and len(t["offset"]) > 200
        cig = t["offset"] + np.uint64(36) + t["l_read_name"].astype(np.uint64)
        seq = cig + np.uint64(4) * t["n_cigar_op"].astype(np.uint64)
        self.rec = dict(pos=t["pos"], flags=t["flag"], contig=t["ref_id"].astype(np.uint32), cigar_off=cig, n_cigar=t["n_cigar_op"].astype(np.uint32), seq_off=seq,
                        l_seq=t["l_seq"], qual_off=seq + ((t["l_seq"].astype(np.uint64) + np.uint64(1)) >> np.uint64(1)))
        tables = pm.read_vcf_tables(prefix + ".vcf", names)
        self.tab = pm.pack_tables([tables[n] for n in names])
        fa = read_fasta(prefix + ".fa")
        self.ref_off = np.cumsum([0] + [len(fa[n]) for n in names]).astype(np.uint64)
        self.ref_seq = np.frombuffer(b"".join(fa[n] for n in names), np.uint8)
        self.n_contigs = len(names)
        self.rec_names = [t["names"][int(t["name_off"][i]):int(t["name_off"][i + 1]) - 1].tobytes() for i in range(len(t["offset"]))]

    def call(self, ctx, blob, refs, walk):
        kw = dict(ref_off=self.ref_off, ref_seq=self.ref_seq, walk=walk) if refs else {}
        return ctx.pileup_records_resident(blob=blob, **self.rec, **self.tab, **kw)

    def plan(self, summary):
        """every name's records as one fragment, in file order (a pair's second mate marked), the fragments in Frag::cmp order: header-sized data only"""
        groups = {}
        for i, nm in enumerate(self.rec_names):
            groups.setdefault((int(self.rec["contig"][i]), nm), []).append(i)
        has = np.diff(summary.cell_off.astype(np.int64)) > 0
        frags = []
        for (ctg, _), idx in groups.items():
            with_cells = [i for i in idx if has[i]]
            if with_cells:
                frags.append((ctg, min(int(summary.first_snp[i]) for i in with_cells), -max(int(summary.last_snp[i]) for i in with_cells), idx[0], idx))
        frags.sort(key=lambda f: f[:4])
        frag_off = np.searchsorted([f[0] for f in frags], np.arange(self.n_contigs + 1)).astype(np.uint64)
        part_off = np.cumsum([0] + [len(f[4]) for f in frags]).astype(np.uint64)
        part_rec = np.array([i for f in frags for i in f[4]], np.uint32)
        mate = np.array([1 if self.rec["flags"][i] & 128 else 0 for i in part_rec], np.uint8)
        return frag_off, part_off, part_rec, mate


def downloads(hip_lib, c):
    out = {}
    ro = c.download("read_off", c.n_reads + 1)
    n_cells = int(ro[-1]) if c.n_reads else 0
    out["read_off"] = ro
    for f, n in (("first", c.n_reads), ("last", c.n_reads), ("snp", n_cells), ("cell_aw", n_cells), ("tw", 2 * c.n_reads), ("meta", 8 * c.n_reads), ("seq_pos", n_cells)):
        out[f] = c.download(f, n)
    try:
        out["set_order"] = c.download("set_order", n_cells)
    except hip_lib.FloriaHipError as e:                         # a contig without a merged fragment carries none
        out["set_order"] = str(e)
    return out


@pytest.mark.parametrize("which", ["hand", "noisy"])
def test_blob_path_equals_the_host_blob_path(gpu_ctx, hip_lib, datasets, which):
    w = World(gpu_ctx, datasets[which])
    flags = capi.FLORIA_ASM_KEEP_SEQ_POS | capi.FLORIA_ASM_DERIVE_SET_ORDER
    try:
        for refs, walk in ((False, None), (True, None), (True, (8, 2, "max", "right"))):
            got, up = {}, {}
            for name, blob in (("host", w.raw), ("handle", w.blob)):
                s = w.call(gpu_ctx, blob, refs, walk)
                t = gpu_ctx.timing()
                up[name] = t["upload_pinned_bytes"] + t["upload_staged_bytes"]
                frag_off, part_off, part_rec, mate = w.plan(s)
                contigs = gpu_ctx.assemble_contigs(s, frag_off, part_off, part_rec, part_mate=mate, _flags=flags)
                got[name] = (s, {f: getattr(s, f).copy() for f in SUMMARY}, dict(s.counts), [downloads(hip_lib, c) for c in contigs], (frag_off, part_off, part_rec))
                for c in contigs:
                    c.free()
                s.free()
            assert up["host"] - up["handle"] == w.blob.nbytes > 0, up                 # the arrays and tables alone: no record byte went up
            (_, hs, hc, hd, hp), (_, bs, bc, bd, bp) = got["host"], got["handle"]
            assert hc == bc and hc["cells"] > 1000 and (not refs or hc["in_bounds"] > 0), (which, refs, walk, hc, bc)
            for f in SUMMARY:
                assert np.array_equal(hs[f], bs[f]), (which, refs, walk, f)
            assert all(np.array_equal(a, b) for a, b in zip(hp, bp))
            assert len(hd) == len(bd) == w.n_contigs
            for a, b in zip(hd, bd):
                assert len(a["snp"]) > 0 and isinstance(a["set_order"], str) == (which == "noisy")      # the hand-built set holds merged fragments: its contig carries a derived set_order
                for f in a:
                    assert np.array_equal(a[f], b[f]), (which, refs, walk, f)
    finally:
        w.blob.free()


def test_refusals(gpu_ctx, hip_lib, datasets):
    w = World(gpu_ctx, datasets["hand"])
    L = hip_lib.load()
    try:
        want = w.call(gpu_ctx, w.blob, False, None)
        want_off = want.cell_off.copy()
        want.free()

        def still_serves():
            s = w.call(gpu_ctx, w.blob, False, None)
            assert np.array_equal(s.cell_off, want_off)
            s.free()
        # an offset past the handle
        bad = dict(w.rec)
        bad["qual_off"] = w.rec["qual_off"].copy()
        bad["qual_off"][7] = w.blob.nbytes - 1
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            gpu_ctx.pileup_records_resident(blob=w.blob, **bad, **w.tab)
        assert ei.value.code == -1 and "quality bytes of record 7" in str(ei.value) and str(w.blob.nbytes) in str(ei.value)
        still_serves()
        # a handle of another context
        other = hip_lib.FloriaHip(0)
        with pytest.raises(hip_lib.FloriaHipError) as ei:
            w.call(other, w.blob, False, None)
        assert ei.value.code == -1 and "another context" in str(ei.value)
        other.close()
        still_serves()
        # a non-NULL alignments->blob beside a handle (the mirror never passes one: through the C entry point)
        r, t = w.rec, w.tab
        keep = [np.ascontiguousarray(r[k], dt) for k, dt in (("pos", np.int32), ("flags", np.uint16), ("contig", np.uint32), ("cigar_off", np.uint64), ("n_cigar", np.uint32),
                                                            ("seq_off", np.uint64), ("l_seq", np.uint32), ("qual_off", np.uint64))]
        types = (C.c_int32, C.c_uint16, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64)
        A = capi.CAlignments(capi.ptr(w.raw, C.c_uint8), w.raw.size, len(keep[0]), *[capi.ptr(a, ct) for a, ct in zip(keep, types)])
        tk = [np.ascontiguousarray(t["snp_off"], np.uint64), np.ascontiguousarray(t["snp_pos"], np.int64), np.ascontiguousarray(t["alleles"], np.uint8), np.ascontiguousarray(t["n_alleles"], np.uint8)]
        S = capi.CSnpTable(len(tk[0]) - 1, capi.ptr(tk[0], C.c_uint64), capi.ptr(tk[1], C.c_int64), capi.ptr(tk[2], C.c_uint8), capi.ptr(tk[3], C.c_uint8))
        out = C.POINTER(capi.CRecordSummary)()
        rc = L.floria_hip_pileup_records_resident_blob(gpu_ctx._h, w.blob._h, C.byref(A), C.byref(S), None, None, C.byref(out))
        assert rc == -1 and not out and b"blob must be NULL" in L.floria_hip_last_error()
        A.blob = None
        rc = L.floria_hip_pileup_records_resident_blob(gpu_ctx._h, w.blob._h, C.byref(A), C.byref(S), None, None, C.byref(out))
        assert rc == 0 and out
        assert np.array_equal(capi.np_from(out.contents.cell_off, len(keep[0]) + 1, np.uint64), want_off)
        L.floria_hip_record_summary_free(out)
    finally:
        w.blob.free()
