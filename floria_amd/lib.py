"""ctypes binding of libfloria_hip.so (include/floria_hip.h) — the Python mirror of the two reference
seams: `generate_hap_graph`'s per-block loop (graph_processing.rs:325-372) and
`process_reads_for_final_parts` (part_block_manip.rs:174-274).

No fallback: if the shared library is missing or no HIP device is usable, everything here raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _capi as capi
from .pileup import Pileup

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.path.join(_CSRC, "libfloria_hip.so")
_LIB = None

# every symbol include/floria_hip.h declares
SYMBOLS = [
    "floria_hip_create", "floria_hip_destroy", "floria_hip_last_error", "floria_hip_version", "floria_hip_init_env", "floria_hip_realign", "floria_hip_realign_walk", "floria_hip_selftest",
    "floria_hip_block_ranges", "floria_hip_ranges_free", "floria_hip_contig_upload", "floria_hip_contig_free",
    "floria_hip_phase_blocks_resident", "floria_hip_phase_blocks", "floria_hip_block_result_free",
    "floria_hip_phase_blocks_batch", "floria_hip_reassign", "floria_hip_groups_free", "floria_hip_last_timing",
    "floria_hip_set_slots", "floria_hip_reassign_batch", "floria_hip_groups_array_free",
    "floria_hip_hap_graph", "floria_hip_hap_graph_free", "floria_hip_reassign_ordered", "floria_hip_haploset_stats",
    "floria_hip_hapq", "floria_hip_hapq_batch",
    "floria_hip_contig_upload_batch", "floria_hip_host_alloc", "floria_hip_host_free", "floria_hip_set_option",
    "floria_hip_contig_download", "floria_hip_phase_pileups_batch",
    "floria_hip_pileup_records", "floria_hip_record_cells_free", "floria_hip_pileup_records_realign",
    "floria_hip_pileup_records_resident", "floria_hip_record_summary_free", "floria_hip_assemble_contigs", "floria_hip_assemble_contigs_ordered", "floria_hip_haploset_alleles",
    "floria_hip_assemble_contigs_opt", "floria_hip_read_spans",
    "floria_hip_drop_monomorphic", "floria_hip_mono_result_free", "floria_hip_mono_timing",
    "floria_hip_reassign_batch_resident", "floria_hip_haplosets_free", "floria_hip_haplosets_download", "floria_hip_haploset_stats_resident", "floria_hip_hapq_batch_resident",
    "floria_hip_haploset_alleles_resident", "floria_hip_read_spans_resident", "floria_hip_join_paths", "floria_hip_reassign_haplosets_resident",
    "floria_hip_inflate_bgzf", "floria_hip_blob_bytes", "floria_hip_blob_download", "floria_hip_blob_free", "floria_hip_blob_records", "floria_hip_blob_records_free",
    "floria_hip_pileup_records_resident_blob", "floria_hip_blob_records_opt", "floria_hip_blob_sequences", "floria_hip_blob_sequences_free",
    "floria_hip_blob_estimate", "floria_hip_estimate_result_free",
    "floria_hip_pack_bytes", "floria_hip_pack_pileup", "floria_hip_pack_bytes_batch", "floria_hip_pack_pileups_batch", "floria_hip_contig_upload_batch_packed", "floria_hip_phase_pileups_batch_packed",
]


class FloriaHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfloria_hip rc={code}: {msg}")
        self.code = code


def build(force=False):
    """Compile libfloria_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).  make decides whether the library is
    stale (every *.h of csrc/ and include/floria_hip.h are prerequisites); where no hipcc exists (the GPU box gets the prebuilt
    library with the snapshot) an existing library is used as it is."""
    import shutil
    have_hipcc = os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")
    if not have_hipcc and os.path.exists(_SO):
        return _SO
    subprocess.check_call(["make", "-C", _CSRC] + (["-B"] if force else []) + ["libfloria_hip.so"], stdout=subprocess.DEVNULL)
    return _SO


def load():
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")      # streams of the job groups / upload pipeline on separate hardware queues (read when HIP initialises)
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise FloriaHipError(-2, f"{_SO} is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(_SO)
        L.floria_hip_last_error.restype = C.c_char_p
        L.floria_hip_version.restype = C.c_char_p
        for s in ("floria_hip_destroy", "floria_hip_ranges_free", "floria_hip_contig_free", "floria_hip_block_result_free", "floria_hip_groups_free",
                  "floria_hip_groups_array_free", "floria_hip_hap_graph_free", "floria_hip_record_cells_free", "floria_hip_record_summary_free", "floria_hip_mono_result_free"):
            getattr(L, s).restype = None
        L.floria_hip_destroy.argtypes = [C.c_void_p]
        L.floria_hip_contig_free.argtypes = [C.c_void_p]
        L.floria_hip_host_alloc.restype = C.c_void_p
        L.floria_hip_host_alloc.argtypes = [C.c_size_t]
        L.floria_hip_host_free.restype = None
        L.floria_hip_host_free.argtypes = [C.c_void_p]
        L.floria_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.floria_hip_pack_bytes.restype = C.c_size_t
        L.floria_hip_pack_bytes.argtypes = [C.c_void_p]
        L.floria_hip_pack_bytes_batch.restype = C.c_size_t
        L.floria_hip_pack_bytes_batch.argtypes = [C.c_void_p, C.c_uint32]
        L.floria_hip_pack_pileups_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.floria_hip_pack_pileup.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.floria_hip_pileup_records.argtypes = [C.c_void_p, C.POINTER(capi.CAlignments), C.POINTER(capi.CSnpTable), C.POINTER(C.POINTER(capi.CRecordCells))]
        L.floria_hip_record_cells_free.argtypes = [C.POINTER(capi.CRecordCells)]
        L.floria_hip_pileup_records_realign.argtypes = [C.c_void_p, C.POINTER(capi.CAlignments), C.POINTER(capi.CSnpTable), C.POINTER(capi.CRefSeqs), C.POINTER(capi.CRealignWalk),
                                                        C.POINTER(C.POINTER(capi.CRecordCells)), C.POINTER(capi.CRealignCounts)]
        L.floria_hip_pileup_records_resident.argtypes = [C.c_void_p, C.POINTER(capi.CAlignments), C.POINTER(capi.CSnpTable), C.POINTER(capi.CRefSeqs), C.POINTER(capi.CRealignWalk),
                                                         C.POINTER(C.POINTER(capi.CRecordSummary))]
        L.floria_hip_record_summary_free.argtypes = [C.POINTER(capi.CRecordSummary)]
        L.floria_hip_assemble_contigs.argtypes = [C.c_void_p, C.POINTER(capi.CRecordSummary), C.POINTER(capi.CFragmentPlan), C.POINTER(C.c_void_p)]
        L.floria_hip_assemble_contigs_ordered.argtypes = [C.c_void_p, C.POINTER(capi.CRecordSummary), C.POINTER(capi.CFragmentPlan), C.POINTER(C.c_void_p)]
        L.floria_hip_assemble_contigs_opt.argtypes = [C.c_void_p, C.POINTER(capi.CRecordSummary), C.POINTER(capi.CFragmentPlan), C.POINTER(capi.CAssembleOptions), C.POINTER(C.c_void_p)]
        L.floria_hip_read_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, capi.u32p, capi.u64p, capi.u32p, capi.u32p, C.c_uint32, capi.u32p, capi.u32p]
        L.floria_hip_drop_monomorphic.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, capi.u64p, C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(capi.CMonoResult))]
        L.floria_hip_mono_result_free.argtypes = [C.POINTER(capi.CMonoResult)]
        L.floria_hip_mono_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.floria_hip_haploset_alleles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, capi.u32p, capi.u64p, capi.u32p, capi.u32p, C.c_uint32, capi.u64p, capi.u32p]
        L.floria_hip_reassign_batch_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, capi.u32p, capi.u64p, capi.u32p, capi.u32p, C.c_uint32, capi.u32p, capi.u64p, C.c_double,
                                                         C.POINTER(C.c_void_p)]
        L.floria_hip_haplosets_free.restype = None
        L.floria_hip_haplosets_free.argtypes = [C.c_void_p]
        L.floria_hip_haplosets_download.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.POINTER(capi.CGroups)))]
        L.floria_hip_haploset_stats_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, capi.f64p]
        L.floria_hip_hapq_batch_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, capi.u32p, C.c_uint64, capi.u8p, capi.f64p, capi.f64p]
        L.floria_hip_haploset_alleles_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, capi.u64p, capi.u32p]
        L.floria_hip_read_spans_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, capi.u32p, capi.u32p]
        L.floria_hip_join_paths.argtypes = [C.c_void_p, C.POINTER(capi.CBlockResult), C.c_void_p, C.c_uint32, capi.u32p, capi.u64p, capi.u32p, capi.u8p, capi.u32p, C.c_uint32,
                                            C.POINTER(C.c_void_p)]
        L.floria_hip_reassign_haplosets_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.POINTER(C.c_void_p)]
        L.floria_hip_inflate_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, capi.u64p, capi.u32p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.floria_hip_blob_bytes.restype = C.c_uint64
        L.floria_hip_blob_bytes.argtypes = [C.c_void_p]
        L.floria_hip_blob_download.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.floria_hip_blob_free.restype = None
        L.floria_hip_blob_free.argtypes = [C.c_void_p]
        L.floria_hip_blob_records.argtypes = [C.c_void_p, C.c_void_p, capi.u64p, capi.u64p, C.c_uint32, C.POINTER(C.POINTER(capi.CBlobRecords))]
        L.floria_hip_blob_records_opt.argtypes = [C.c_void_p, C.c_void_p, capi.u64p, capi.u64p, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(capi.CBlobRecords))]
        L.floria_hip_blob_sequences.argtypes = [C.c_void_p, C.c_void_p, capi.u64p, capi.u32p, capi.u64p, C.c_uint64, C.POINTER(C.POINTER(capi.CBlobSequences))]
        L.floria_hip_blob_sequences_free.restype = None
        L.floria_hip_blob_sequences_free.argtypes = [C.POINTER(capi.CBlobSequences)]
        L.floria_hip_blob_estimate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.CEstimateRecords), C.c_uint32, C.POINTER(capi.CEstimateState), C.POINTER(C.POINTER(capi.CEstimateResult))]
        L.floria_hip_estimate_result_free.restype = None
        L.floria_hip_estimate_result_free.argtypes = [C.POINTER(capi.CEstimateResult)]
        L.floria_hip_blob_records_free.restype = None
        L.floria_hip_blob_records_free.argtypes = [C.POINTER(capi.CBlobRecords)]
        L.floria_hip_pileup_records_resident_blob.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.CAlignments), C.POINTER(capi.CSnpTable), C.POINTER(capi.CRefSeqs),
                                                              C.POINTER(capi.CRealignWalk), C.POINTER(C.POINTER(capi.CRecordSummary))]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise FloriaHipError(rc, load().floria_hip_last_error().decode())


def make_params(epsilon, max_ploidy=5, beam=10, ploidy_sensitivity=2, stopping_heuristic=1):
    """The hot-path fields of `Options` (types_structs.rs:20-51) with the CLI defaults
    (parse_cmd_line.rs: -p 5, -n 10, -s 2, stopping heuristic on)."""
    return capi.CParams(float(epsilon), int(max_ploidy), int(beam), int(ploidy_sensitivity), int(stopping_heuristic))


def get_range_with_lengths(snp_to_genome_pos, block_length, overlap_len=None, minimal_density=0.0005):
    """utils_frags::get_range_with_lengths (utils_frags.rs:405-463); overlap defaults to block_length/3
    as in generate_hap_graph (graph_processing.rs:334-339).  Returns (start, end) uint32 arrays, 1-based inclusive."""
    g = np.ascontiguousarray(snp_to_genome_pos, np.uint64)
    if overlap_len is None:
        overlap_len = block_length // 3
    out = C.POINTER(capi.CRanges)()
    _check(load().floria_hip_block_ranges(capi.ptr(g, C.c_uint64), C.c_uint32(len(g)), C.c_uint64(block_length), C.c_uint64(overlap_len),
                                          C.c_double(minimal_density), C.byref(out)))
    r = out.contents
    res = (capi.np_from(r.start, r.n, np.uint32), capi.np_from(r.end, r.n, np.uint32))
    load().floria_hip_ranges_free(out)
    return res


class PinnedArena:
    """Pinned host memory (floria_hip_host_alloc) handed out as numpy arrays: pileups whose arrays live here upload by DMA
    with no staging copy, and arrays carved consecutively are back to back, so a batch travels as one transfer per field."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._p = load().floria_hip_host_alloc(C.c_size_t(self.nbytes))
        if not self._p:
            raise FloriaHipError(-3, load().floria_hip_last_error().decode())
        self._buf = (C.c_uint8 * self.nbytes).from_address(self._p)
        self._cursor = 0

    def take(self, count, dtype):
        """Next `count` elements of `dtype` (element-aligned, NOT padded: consecutive takes of one dtype are contiguous)."""
        dt = np.dtype(dtype)
        off = (self._cursor + dt.itemsize - 1) // dt.itemsize * dt.itemsize
        end = off + int(count) * dt.itemsize
        if end > self.nbytes:
            raise MemoryError("PinnedArena exhausted")
        self._cursor = end
        return np.frombuffer(self._buf, dtype=dt, count=int(count), offset=off)

    def free(self):
        if self._p:
            self._buf = None
            load().floria_hip_host_free(C.c_void_p(self._p))
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pin_pileups(pileups):
    """Copy pileups into ONE pinned arena, field by field (all read_off arrays back to back, then all first, ...):
    what a host that marshals `Vec<Frag>` into upload buffers writes directly.  Returns (arena, [Pileup views])."""
    nr = sum(p.n_reads for p in pileups)
    nc = sum(p.n_cells for p in pileups)
    with_order = any(p.set_order is not None for p in pileups)
    arena = PinnedArena(4 * (nr + len(pileups)) + 8 * nr + (10 if with_order else 6) * nc + 256)
    fields = {}
    for name, dt in (("read_off", np.uint32), ("first", np.uint32), ("last", np.uint32), ("snp", np.uint32), ("allele", np.uint8), ("qual", np.uint8)):
        views = []
        for p in pileups:
            src = np.ascontiguousarray(getattr(p, name), dt)
            v = arena.take(len(src), dt)
            v[:] = src
            views.append(v)
        fields[name] = views
    out = [Pileup(fields["read_off"][i], fields["snp"][i], fields["allele"][i], fields["qual"][i], fields["first"][i], fields["last"][i]) for i in range(len(pileups))]
    if with_order:
        for p, o in zip(pileups, out):
            if p.set_order is not None:
                v = arena.take(p.n_cells, np.uint32)
                v[:] = np.ascontiguousarray(p.set_order, np.uint32)
                o.set_order = v
    return arena, out


class _PlainArena:
    """Pageable stand-in for PinnedArena (tests of the host-side packer on machines without a GPU)."""

    def __init__(self, nbytes):
        self._arr = np.zeros(int(nbytes) + 64, np.uint8)
        self._p = self._arr.ctypes.data

    def free(self):
        pass


def pack_pileups(pileups, pinned=True):
    """The compact wire form (floria_pileup_packed) of a list of Pileups, packed by floria_hip_pack_pileup into ONE pinned arena:
    what a host marshals its Vec<Frag> into for the PCIe link.  Returns (arena, ctypes array of floria_pileup_packed, packed bytes)."""
    L = load()
    n = len(pileups)
    carr = c_pileups(pileups)
    size = int(L.floria_hip_pack_bytes_batch(carr, C.c_uint32(n)))
    if n and size == 0:
        raise FloriaHipError(-1, "pileups cannot be packed (null field, last < first, or spans of 2^32 bits and more)")
    arena = (PinnedArena if pinned else _PlainArena)(size + 128)
    arr = (capi.CPileupPacked * n)()
    base = arena._p + (64 - arena._p % 64) % 64
    _check(L.floria_hip_pack_pileups_batch(carr, C.c_uint32(n), C.c_void_p(base), C.c_size_t(size), arr))
    return arena, arr, size


class ResidentContig:
    def __init__(self, ctx, pileup: Pileup = None, handle=None, n_reads=None):
        self.ctx = ctx
        if handle is not None:
            self._h = handle
            self.n_reads = n_reads
            return
        self.n_reads = pileup.n_reads
        cp = pileup.as_c()
        h = C.c_void_p()
        _check(load().floria_hip_contig_upload(ctx._h, C.byref(cp), C.byref(h)))
        self._h = h

    FIELDS = {"read_off": (0, np.uint32), "first": (1, np.uint32), "last": (2, np.uint32), "snp": (3, np.uint32),
              "cell_aw": (4, np.uint32), "tw": (5, np.uint64), "meta": (6, np.uint32), "set_order": (7, np.uint32), "seq_pos": (8, np.uint32)}

    def download(self, field, count):
        """Diagnostic (floria_hip_contig_download): `count` elements of a resident array."""
        fid, dt = self.FIELDS[field]
        out = np.zeros(int(count), dt)
        _check(load().floria_hip_contig_download(self._h, C.c_int(fid), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self._h:
            load().floria_hip_contig_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ContigBatch:
    """The handles of one floria_hip_contig_upload_batch call, kept as the ctypes array the C entry points take (no per-contig
    Python objects: a host loop that uploads and phases batch after batch pays only the C calls)."""

    def __init__(self, ctx, handles, n):
        self.ctx, self._arr, self.n = ctx, handles, n

    def __len__(self):
        return self.n

    def free(self):
        if self._arr is not None:
            L = load()
            for i in range(self.n):
                L.floria_hip_contig_free(C.c_void_p(self._arr[i]))
            self._arr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RecordSummary:
    """floria_record_summary of one FloriaHip.pileup_records_resident call: numpy copies of the per-record arrays (cell_off uint64 [n + 1], first_snp / last_snp
    uint32 [n], ref_end int64 [n]), the realign counts, and the library-owned struct itself, which FloriaHip.assemble_contigs hands back to the library.  The cells
    stay on the device until the context's next pileup_records* call."""

    def __init__(self, ctx, cptr, n):
        self.ctx, self._p = ctx, cptr
        r = cptr.contents
        self.n_records = n
        self.cell_off = capi.np_from(r.cell_off, n + 1, np.uint64)
        self.first_snp = capi.np_from(r.first_snp, n, np.uint32)
        self.last_snp = capi.np_from(r.last_snp, n, np.uint32)
        self.ref_end = capi.np_from(r.ref_end, n, np.int64)
        self.counts = {f: int(getattr(r.counts, f)) for f, _ in capi.CRealignCounts._fields_}
        self.token = int(r.token)

    def free(self):
        if self._p is not None:
            load().floria_hip_record_summary_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Haplosets:
    """floria_hip_haplosets: the result of one FloriaHip.reassign_batch_resident call, resident on the device.  download() -> what reassign_batch returns (a list of
    _capi.Groups in contig order, fetched once and kept); the four consumers take the handle as haplosets= (with the contigs of the S2 call) and upload no group."""

    def __init__(self, ctx, handle, n_contigs):
        self.ctx, self._h, self.n_contigs, self._groups = ctx, handle, n_contigs, None

    def download(self):
        if self._groups is None:
            out = C.POINTER(C.POINTER(capi.CGroups))()
            _check(load().floria_hip_haplosets_download(self._h, C.byref(out)))
            self._groups = [capi.Groups(out[i].contents) for i in range(self.n_contigs)]
            load().floria_hip_groups_array_free(out, C.c_uint32(self.n_contigs))
        return self._groups

    @property
    def n_groups(self):
        return sum(g.n_groups for g in self.download())

    @property
    def n_entries(self):
        return sum(len(g.grp_read) for g in self.download())

    def ranges(self):
        """uint32 [n_groups, 2]: the ranges of all contigs' groups in the handle's order."""
        return np.concatenate([g.range.reshape(-1, 2) for g in self.download()] + [np.zeros((0, 2), np.uint32)])

    def free(self):
        if self._h is not None:
            load().floria_hip_haplosets_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Blob:
    """floria_hip_blob: BGZF members inflated on the device by FloriaHip.inflate_bgzf, back to back.  nbytes; download(off=0, nbytes=None) -> uint8 array; free().
    FloriaHip.blob_records(blob, ...) gives its record table, FloriaHip.pileup_records_resident(blob=blob, ...) walks its records where they lie."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        self.nbytes = int(load().floria_hip_blob_bytes(handle))

    def download(self, off=0, nbytes=None):
        n = self.nbytes - int(off) if nbytes is None else int(nbytes)
        out = np.zeros(max(n, 0), np.uint8)
        _check(load().floria_hip_blob_download(self._h, C.c_uint64(int(off)), out.ctypes.data_as(C.c_void_p), C.c_uint64(max(n, 0))))
        return out

    def free(self):
        if self._h is not None:
            load().floria_hip_blob_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _contig_array(contigs):
    n = len(contigs)
    return contigs._arr if isinstance(contigs, ContigBatch) else (C.c_void_p * max(n, 1))(*[c._h for c in contigs])


def c_pileups(pileups):
    """ctypes array of floria_pileup for a list of Pileups (keep the Pileups alive while it is in use)."""
    return (capi.CPileup * len(pileups))(*[p.as_c() for p in pileups])


class FloriaHip:
    """One context per device (floria_hip_create)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(load().floria_hip_create(C.c_int(device), C.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            load().floria_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_slots(self, n):
        _check(load().floria_hip_set_slots(self._h, C.c_uint32(n)))

    def set_option(self, key, value):
        """floria_hip_set_option.  "arith" = 1 selects the reference's running-sum arithmetic (a different function at an epsilon that is not a
        multiple of 2^-10, slower kernels; include/floria_hip.h); every other key is a tuning / test knob that changes no result."""
        _check(load().floria_hip_set_option(self._h, key.encode(), C.c_int64(int(value))))

    def selftest(self, epsilon, n_max=1024):
        """floria_hip_selftest: max |f32 screen - host table| / n of the binomial p-value on this device."""
        out = C.c_double(0.0)
        fn = load().floria_hip_selftest
        fn.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.POINTER(C.c_double)]
        _check(fn(self._h, C.c_double(epsilon), C.c_uint32(n_max), C.byref(out)))
        return out.value

    def upload(self, pileup: Pileup):
        return ResidentContig(self, pileup)

    def upload_batch(self, pileups):
        """floria_hip_contig_upload_batch: one allocation, DMA of the raw arrays, validate + flatten on the device."""
        n = len(pileups)
        arr = c_pileups(pileups)
        hs = (C.c_void_p * n)()
        _check(load().floria_hip_contig_upload_batch(self._h, arr, C.c_uint32(n), hs))
        return [ResidentContig(self, handle=C.c_void_p(hs[i]), n_reads=pileups[i].n_reads) for i in range(n)]

    def upload_batch_c(self, carr, n=None):
        """The same for a prebuilt ctypes floria_pileup array -> ContigBatch."""
        n = len(carr) if n is None else n
        hs = (C.c_void_p * n)()
        _check(load().floria_hip_contig_upload_batch(self._h, carr, C.c_uint32(n), hs))
        return ContigBatch(self, hs, n)

    def upload_batch_packed(self, parr, n=None):
        """floria_hip_contig_upload_batch_packed for a ctypes floria_pileup_packed array (pack_pileups) -> ContigBatch."""
        n = len(parr) if n is None else n
        hs = (C.c_void_p * n)()
        _check(load().floria_hip_contig_upload_batch_packed(self._h, parr, C.c_uint32(n), hs))
        return ContigBatch(self, hs, n)

    def timing(self):
        t = capi.CTiming()
        _check(load().floria_hip_last_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in capi.CTiming._fields_}

    # S1 --------------------------------------------------------------------------------------------
    def phase_blocks(self, contig, blk_start, blk_end, params):
        """get_local_hap_blocks for every (start,end) SNP range of one contig (graph_processing.rs:345-362)."""
        if isinstance(contig, Pileup):
            rc = self.upload(contig)
            try:
                return self.phase_blocks(rc, blk_start, blk_end, params)
            finally:
                rc.free()
        bs = np.ascontiguousarray(blk_start, np.uint32)
        be = np.ascontiguousarray(blk_end, np.uint32)
        out = C.POINTER(capi.CBlockResult)()
        _check(load().floria_hip_phase_blocks_resident(self._h, contig._h, capi.ptr(bs, C.c_uint32), capi.ptr(be, C.c_uint32),
                                                       C.c_uint32(len(bs)), C.byref(params), C.byref(out)))
        res = capi.BlockResult(out.contents)
        load().floria_hip_block_result_free(out)
        return res

    def phase_blocks_batch(self, contigs, blk_contig, blk_start, blk_end, params, copy_out=True):
        arr = contigs._arr if isinstance(contigs, ContigBatch) else (C.c_void_p * len(contigs))(*[c._h for c in contigs])
        bc = np.ascontiguousarray(blk_contig, np.uint32)
        bs = np.ascontiguousarray(blk_start, np.uint32)
        be = np.ascontiguousarray(blk_end, np.uint32)
        out = C.POINTER(capi.CBlockResult)()
        _check(load().floria_hip_phase_blocks_batch(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(bc, C.c_uint32), capi.ptr(bs, C.c_uint32),
                                                    capi.ptr(be, C.c_uint32), C.c_uint32(len(bs)), C.byref(params), C.byref(out)))
        res = capi.BlockResult(out.contents) if copy_out else None
        load().floria_hip_block_result_free(out)
        return res

    def phase_pileups_batch(self, pileups, blk_contig, blk_start, blk_end, params, keep=False, copy_out=True):
        """floria_hip_phase_pileups_batch: S1 straight from host pileups (a list of Pileups or a prebuilt c_pileups array),
        transfers pipelined with the kernels.  Returns the BlockResult, or (BlockResult, ContigBatch) with keep=True."""
        carr = pileups if isinstance(pileups, C.Array) else c_pileups(pileups)
        n = len(carr)
        packed = isinstance(carr, C.Array) and carr._type_ is capi.CPileupPacked          # (pack_pileups: the compact wire form)
        bc = np.ascontiguousarray(blk_contig, np.uint32)
        bs = np.ascontiguousarray(blk_start, np.uint32)
        be = np.ascontiguousarray(blk_end, np.uint32)
        out = C.POINTER(capi.CBlockResult)()
        hs = (C.c_void_p * n)() if keep else None
        fn = load().floria_hip_phase_pileups_batch_packed if packed else load().floria_hip_phase_pileups_batch
        _check(fn(self._h, carr, C.c_uint32(n), capi.ptr(bc, C.c_uint32), capi.ptr(bs, C.c_uint32),
                  capi.ptr(be, C.c_uint32), C.c_uint32(len(bs)), C.byref(params), C.byref(out), hs))
        res = capi.BlockResult(out.contents) if copy_out else None
        load().floria_hip_block_result_free(out)
        return (res, ContigBatch(self, hs, n)) if keep else res

    def hap_graph(self, res):
        """HapNode::new coverage + update_hap_graph out_weights (graph_processing.rs:22-100) for the batch that produced
        `res`; must directly follow the phase_blocks* call on this context (the batch is still resident in HBM)."""
        bp = np.ascontiguousarray(res.best_ploidy, np.uint32)
        c = capi.CBlockResult()
        c.n_blocks = res.n_blocks; c.max_ploidy = res.max_ploidy; c.best_ploidy = capi.ptr(bp, C.c_uint32); c.batch_token = res.batch_token
        out = C.POINTER(capi.CHapGraph)()
        _check(load().floria_hip_hap_graph(self._h, C.byref(c), C.byref(out)))
        g = capi.HapGraph(out.contents)
        load().floria_hip_hap_graph_free(out)
        return g

    def haploset_stats(self, contigs, grp_contig=None, groups=None, ranges=None, haplosets=None):
        """get_errors_cov_from_frags (utils_frags.rs:596-655) per haploset -> float64 [n_groups, 4] = cov, err, total_err, total_cov.
        haplosets= a Haplosets handle made from `contigs`: its groups, nothing uploaded."""
        if haplosets is not None:
            out = np.zeros((haplosets.n_groups, 4), np.float64)
            _check(load().floria_hip_haploset_stats_resident(self._h, _contig_array(contigs), C.c_uint32(len(contigs)), haplosets._h, capi.ptr(out, C.c_double)))
            return out
        arr = (C.c_void_p * len(contigs))(*[c._h for c in contigs])
        gc = np.ascontiguousarray(grp_contig, np.uint32)
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if len(groups) else np.zeros(0, np.uint32), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        out = np.zeros((len(groups), 4), np.float64)
        _check(load().floria_hip_haploset_stats(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64),
                                                capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32), C.c_uint32(len(groups)), capi.ptr(out, C.c_double)))
        return out

    def hapq(self, contig, groups, ranges, snp_to_genome_pos, block_length):
        """get_hapq (part_block_manip.rs:517-616) for one contig's haplosets -> (hapq uint8 [n], rel_err float64 [n], avg_err)."""
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if len(groups) else np.zeros(0, np.uint32), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        pos = np.ascontiguousarray(snp_to_genome_pos, np.uint64)
        hq = np.zeros(len(groups), np.uint8)
        rel = np.zeros(len(groups), np.float64)
        avg = C.c_double(0)
        _check(load().floria_hip_hapq(self._h, contig._h, capi.ptr(off, C.c_uint64), capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32),
                                      C.c_uint32(len(groups)), capi.ptr(pos, C.c_uint64), C.c_uint32(len(pos)), C.c_uint64(int(block_length)),
                                      capi.ptr(hq, C.c_uint8), capi.ptr(rel, C.c_double), C.byref(avg)))
        return hq, rel, avg.value

    def realign(self, read_windows, ref_windows, alleles, n_alleles, want_scores=False):
        """alignment::realign for n SNP calls: read_windows / ref_windows uint8 [n, 32], alleles uint8 [n, 4], n_alleles uint8 [n]
        -> best allele index uint8 [n] (and the best score int32 [n])."""
        q = np.ascontiguousarray(read_windows, np.uint8); r = np.ascontiguousarray(ref_windows, np.uint8)
        al = np.ascontiguousarray(alleles, np.uint8); na = np.ascontiguousarray(n_alleles, np.uint8)
        n = len(na)
        assert q.shape == (n, 32) and r.shape == (n, 32) and al.shape == (n, 4)
        best = np.zeros(n, np.uint8)
        score = np.zeros(n, np.int32) if want_scores else None
        _check(load().floria_hip_realign(self._h, capi.ptr(q, C.c_uint8), capi.ptr(r, C.c_uint8), capi.ptr(al, C.c_uint8), capi.ptr(na, C.c_uint8), C.c_uint64(n),
                                         capi.ptr(best, C.c_uint8), capi.ptr(score, C.c_int32) if want_scores else None))
        return (best, score) if want_scores else best

    def realign_walk(self, read_windows, ref_windows, alleles, n_alleles, step, rule, tie, want_scores=False, block=8):
        """realign() scored by one member of the fixed-block walk family instead of the exact DP (floria_hip_realign_walk): block 8, step 1 | 2 | 4 | 8,
        rule 0 / "max" | 1 / "sum", tie 0 / "right" | 1 / "down"; any other member raises FloriaHipError (FLORIA_E_INVALID)."""
        q = np.ascontiguousarray(read_windows, np.uint8); r = np.ascontiguousarray(ref_windows, np.uint8)
        al = np.ascontiguousarray(alleles, np.uint8); na = np.ascontiguousarray(n_alleles, np.uint8)
        n = len(na)
        assert q.shape == (n, 32) and r.shape == (n, 32) and al.shape == (n, 4)
        walk = capi.CRealignWalk(int(block), int(step), {"max": 0, "sum": 1}.get(rule, rule), {"right": 0, "down": 1}.get(tie, tie))
        best = np.zeros(n, np.uint8)
        score = np.zeros(n, np.int32) if want_scores else None
        _check(load().floria_hip_realign_walk(self._h, capi.ptr(q, C.c_uint8), capi.ptr(r, C.c_uint8), capi.ptr(al, C.c_uint8), capi.ptr(na, C.c_uint8), C.c_uint64(n),
                                              C.byref(walk), capi.ptr(best, C.c_uint8), capi.ptr(score, C.c_int32) if want_scores else None))
        return (best, score) if want_scores else best

    def pileup_records(self, blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles):
        """floria_hip_pileup_records: frag_from_record (file_reader.rs:661-736) for n alignment records given as offsets into one byte `blob`
        (pos int32 [n], flags uint16 [n], contig uint32 [n], cigar_off / seq_off / qual_off uint64 [n], n_cigar / l_seq uint32 [n]) against a SNP table
        (snp_off uint64 [n_contigs + 1], snp_pos int64, alleles uint8 [n_snps, 4], n_alleles uint8) -> numpy arrays
        (cell_off uint64 [n + 1], snp uint32, allele uint8, qual uint8, seq_pos uint32, ref_end int64 [n]).  Arrays that live in a PinnedArena go up by DMA."""
        return self._pileup_records(blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles)

    def pileup_records_realign(self, blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles, ref_off, ref_seq, walk=None):
        """floria_hip_pileup_records_realign: pileup_records() with alignment::realign applied to the cells on the device.  ref_off uint64 [n_contigs + 1] and ref_seq
        uint8 (or bytes) hold one reference sequence per contig of the SNP table (an empty one: the contig's cells stay as walked; ref_seq None: a null pointer); walk None = the exact DP, or
        (step, rule, tie) / (block, step, rule, tie) as realign_walk() takes them.  -> (the six arrays of pileup_records, dict(cells, in_bounds, shortcut, scored, changed))."""
        return self._pileup_records(blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles, refs=(ref_off, ref_seq), walk=walk)

    def pileup_records_resident(self, blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles, ref_off=None, ref_seq=None, walk=None):
        """floria_hip_pileup_records_resident: pileup_records() (ref_off None) or pileup_records_realign() whose cells stay on the device -> RecordSummary
        (free() it when the fragments are assembled).  Any later pileup_records* call on this context ends the residency.
        blob= a Blob (inflate_bgzf): floria_hip_pileup_records_resident_blob, the offsets index the handle and no record byte is uploaded."""
        return self._pileup_records(blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles,
                                    refs=None if ref_off is None else (ref_off, ref_seq), walk=walk, resident=True)

    def inflate_bgzf(self, file_bytes, member_off, member_bytes):
        """floria_hip_inflate_bgzf: the BGZF members (member_off uint64 [n], member_bytes uint32 [n]) of the file image `file_bytes` (bytes or a uint8 array; one
        that lives in a PinnedArena goes up by DMA) inflated on the device -> Blob, the inflated bytes back to back in the order given."""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        mo = np.ascontiguousarray(member_off, np.uint64); mb = np.ascontiguousarray(member_bytes, np.uint32)
        if len(mo) != len(mb):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "inflate_bgzf: one length per member offset")
        h = C.c_void_p()
        _check(load().floria_hip_inflate_bgzf(self._h, fb.ctypes.data_as(C.c_void_p), C.c_uint64(fb.size), capi.ptr(mo, C.c_uint64), capi.ptr(mb, C.c_uint32), C.c_uint32(len(mo)), C.byref(h)))
        return Blob(self, h)

    def blob_records(self, blob, begin, end, flags=0):
        """floria_hip_blob_records: the record table of a Blob of BAM alignment records, chain c following the block_size prefixes from begin[c] while a whole
        record fits before end[c] -> dict of numpy arrays (chain_rec_off uint64 [n_chains + 1], chain_stop uint64 [n_chains]; per record offset uint64, block_size,
        ref_id, pos, l_seq, cigar0, flag, n_cigar_op, mapq, l_read_name; name_off uint64 [n + 1] and names uint8, the names as stored, NUL included).
        Always through floria_hip_blob_records_opt (flags = 0 is floria_hip_blob_records; else capi.FLORIA_CHAIN_CUT_TAIL | FLORIA_CHAIN_ONE_REF); chain_why uint32
        [n_chains] (0 end, 1 cut tail, 2 another reference) is in the dict."""
        b = np.ascontiguousarray(np.atleast_1d(begin), np.uint64); e = np.ascontiguousarray(np.atleast_1d(end), np.uint64)
        if len(b) != len(e):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "blob_records: one end per begin")
        out = C.POINTER(capi.CBlobRecords)()
        _check(load().floria_hip_blob_records_opt(self._h, blob._h, capi.ptr(b, C.c_uint64), capi.ptr(e, C.c_uint64), C.c_uint32(len(b)), C.c_uint32(int(flags)), C.byref(out)))
        return self._blob_records_result(out)

    @staticmethod
    def _blob_records_result(out):
        """the dict of blob_records from the library's floria_blob_records, which it frees"""
        r = out.contents
        n, nch = int(r.n_records), int(r.n_chains)
        res = dict(chain_rec_off=capi.np_from(r.chain_rec_off, nch + 1, np.uint64), chain_stop=capi.np_from(r.chain_stop, nch, np.uint64), name_off=capi.np_from(r.name_off, n + 1, np.uint64),
                   chain_why=capi.np_from(r.chain_why, nch, np.uint32))
        for f, dt in (("offset", np.uint64), ("block_size", np.uint32), ("ref_id", np.int32), ("pos", np.int32), ("l_seq", np.uint32), ("cigar0", np.uint32), ("flag", np.uint16),
                      ("n_cigar_op", np.uint16), ("mapq", np.uint8), ("l_read_name", np.uint8)):
            res[f] = capi.np_from(getattr(r, f), n, dt)
        res["names"] = capi.np_from(r.names, int(res["name_off"][n]), np.uint8)
        load().floria_hip_blob_records_free(out)
        return res

    def blob_sequences(self, blob, seq_off, l_seq, qual_off):
        """floria_hip_blob_sequences: the bases ('A' 'C' 'G' 'T' for the codes 1 2 4 8, 'A' otherwise) and qualities (q > 222 ? 255 : q + 33) of n records of a
        Blob, record i with its packed bases at seq_off[i] and its l_seq[i] quality bytes at qual_off[i] -> (base_off uint64 [n + 1], bases uint8, quals uint8)."""
        so = np.ascontiguousarray(np.atleast_1d(seq_off), np.uint64); ls = np.ascontiguousarray(np.atleast_1d(l_seq), np.uint32)
        qo = np.ascontiguousarray(np.atleast_1d(qual_off), np.uint64)
        if not len(so) == len(ls) == len(qo):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "blob_sequences: one sequence offset, length and quality offset per record")
        out = C.POINTER(capi.CBlobSequences)()
        _check(load().floria_hip_blob_sequences(self._h, blob._h, capi.ptr(so, C.c_uint64), capi.ptr(ls, C.c_uint32), capi.ptr(qo, C.c_uint64), C.c_uint64(len(so)), C.byref(out)))
        r = out.contents
        base_off = capi.np_from(r.base_off, int(r.n) + 1, np.uint64)
        res = (base_off, capi.np_from(r.bases, int(base_off[-1]), np.uint8), capi.np_from(r.quals, int(base_off[-1]), np.uint8))
        load().floria_hip_blob_sequences_free(out)
        return res

    def blob_estimate(self, blob, pos, cigar_off, n_cigar, seq_off, l_seq, group_off, stop=1000, count=0, n_err=0):
        """floria_hip_blob_estimate: the -e / -l estimate's sampled pileup columns over the (already filtered) records of a Blob, one group per contig (group_off
        uint64 [n_groups + 1]), ascending by pos inside a group; (count, n_err) is the state carried in from the records in front.  -> dict(col_group uint32,
        col_pos int32, col_total uint32, col_most uint32: every sampled column in order; rec_hits uint32 [n]; done bool; count, n_err: the state carried out)."""
        ps = np.ascontiguousarray(np.atleast_1d(pos), np.int32); co = np.ascontiguousarray(np.atleast_1d(cigar_off), np.uint64); nc = np.ascontiguousarray(np.atleast_1d(n_cigar), np.uint32)
        so = np.ascontiguousarray(np.atleast_1d(seq_off), np.uint64); ls = np.ascontiguousarray(np.atleast_1d(l_seq), np.uint32); go = np.ascontiguousarray(np.atleast_1d(group_off), np.uint64)
        if not len(ps) == len(co) == len(nc) == len(so) == len(ls) or len(go) < 1:
            raise FloriaHipError(capi.FLORIA_E_INVALID, "blob_estimate: one pos, CIGAR offset and count, sequence offset and length per record, and n_groups + 1 group offsets")
        recs = capi.CEstimateRecords(len(ps), capi.ptr(ps, C.c_int32), capi.ptr(co, C.c_uint64), capi.ptr(nc, C.c_uint32), capi.ptr(so, C.c_uint64), capi.ptr(ls, C.c_uint32),
                                     len(go) - 1, capi.ptr(go, C.c_uint64))
        state = capi.CEstimateState(int(count), int(n_err))
        out = C.POINTER(capi.CEstimateResult)()
        _check(load().floria_hip_blob_estimate(self._h, blob._h, C.byref(recs), C.c_uint32(int(stop)), C.byref(state), C.byref(out)))
        r = out.contents
        k = int(r.n_cols)
        res = dict(col_group=capi.np_from(r.col_group, k, np.uint32), col_pos=capi.np_from(r.col_pos, k, np.int32), col_total=capi.np_from(r.col_total, k, np.uint32),
                   col_most=capi.np_from(r.col_most, k, np.uint32), rec_hits=capi.np_from(r.rec_hits, len(ps), np.uint32), done=bool(r.done), count=int(state.count), n_err=int(state.n_err))
        load().floria_hip_estimate_result_free(out)
        return res

    def assemble_contigs_ordered(self, summary, frag_off, part_off, part_rec):
        """floria_hip_assemble_contigs_ordered: assemble_contigs() whose merged contigs (a fragment with two or more parts that have cells) carry the set_order
        the reference's containers give their reads, derived on the device (download field "set_order"); the other contigs carry none."""
        return self.assemble_contigs(summary, frag_off, part_off, part_rec, _ordered=True)

    def assemble_contigs(self, summary, frag_off, part_off, part_rec, set_order=None, _ordered=False, keep_seq_pos=False, part_mate=None, _flags=None):
        """floria_hip_assemble_contigs: the fragment plan (frag_off uint64 [n_contigs + 1], part_off uint64 [n_frags + 1], part_rec uint32 record indices in merge
        order, optional set_order uint32 over the merged cells of all contigs) -> one ResidentContig per contig, usable wherever uploaded ones are.
        keep_seq_pos (floria_hip_assemble_contigs_opt, FLORIA_ASM_KEEP_SEQ_POS): every contig also carries one SEQ_POS word `mate << 31 | seq_pos` per cell
        (download field "seq_pos", read_spans); part_mate uint8 [len(part_rec)] marks the parts of the second mate, None = all 0.  (_flags: the raw flags word.)"""
        fo = np.ascontiguousarray(frag_off, np.uint64); po = np.ascontiguousarray(part_off, np.uint64); pr = np.ascontiguousarray(part_rec, np.uint32)
        if len(fo) < 1 or len(po) != int(fo[-1]) + 1 or (len(po) and len(pr) < int(po.max())):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "assemble_contigs: frag_off needs n_contigs + 1 entries, part_off n_frags + 1, part_rec part_off[-1]")
        so = None if set_order is None else np.ascontiguousarray(set_order, np.uint32)
        n = len(fo) - 1
        plan = capi.CFragmentPlan(n, capi.ptr(fo, C.c_uint64), capi.ptr(po, C.c_uint64), capi.ptr(pr, C.c_uint32), None if so is None else capi.ptr(so, C.c_uint32))
        hs = (C.c_void_p * max(n, 1))()
        if summary._p is None:
            raise FloriaHipError(capi.FLORIA_E_INVALID, "assemble_contigs: the record summary has been freed")
        if keep_seq_pos or part_mate is not None or _flags is not None:
            pm = None if part_mate is None else np.ascontiguousarray(part_mate, np.uint8)
            if pm is not None and len(pm) != len(pr):
                raise FloriaHipError(capi.FLORIA_E_INVALID, "assemble_contigs: part_mate needs one byte per entry of part_rec")
            flags = _flags if _flags is not None else (capi.FLORIA_ASM_KEEP_SEQ_POS if keep_seq_pos else 0) | (capi.FLORIA_ASM_DERIVE_SET_ORDER if _ordered else 0)
            opts = capi.CAssembleOptions(int(flags), None if pm is None else capi.ptr(pm, C.c_uint8))
            _check(load().floria_hip_assemble_contigs_opt(self._h, summary._p, C.byref(plan), C.byref(opts), hs))
        else:
            _check((load().floria_hip_assemble_contigs_ordered if _ordered else load().floria_hip_assemble_contigs)(self._h, summary._p, C.byref(plan), hs))
        return [ResidentContig(self, handle=C.c_void_p(hs[i]), n_reads=int(fo[i + 1] - fo[i])) for i in range(n)]

    def drop_monomorphic(self, contigs, snp_counts, error, with_set_order=False):
        """floria_hip_drop_monomorphic: remove_monomorphic_allele (utils_frags.rs:713-772) on resident contigs (a list of ResidentContigs or a ContigBatch) whose
        SNP counts are snp_counts -> (ContigBatch of the filtered contigs, dict(read_off uint64 [n + 1], old_read uint32, removed uint8 [sum of snp_counts],
        n_removed_snps, n_removed_cells, n_dropped_reads, new_first / new_last uint32 [reads of the result]: the survivors' first / last SNP)).  The inputs stay as they are."""
        n = len(contigs)
        arr = contigs._arr if isinstance(contigs, ContigBatch) else (C.c_void_p * max(n, 1))(*[c._h for c in contigs])
        if len(np.atleast_1d(snp_counts)) != n:
            raise FloriaHipError(capi.FLORIA_E_INVALID, "drop_monomorphic: one SNP count per contig")
        so = np.zeros(n + 1, np.uint64)
        so[1:] = np.cumsum(np.asarray(snp_counts, np.uint64), dtype=np.uint64)
        hs = (C.c_void_p * max(n, 1))()
        out = C.POINTER(capi.CMonoResult)()
        _check(load().floria_hip_drop_monomorphic(self._h, arr, C.c_uint32(n), capi.ptr(so, C.c_uint64), C.c_double(error), C.c_int(1 if with_set_order else 0), hs, C.byref(out)))
        r = out.contents
        read_off = capi.np_from(r.read_off, n + 1, np.uint64)
        result = dict(read_off=read_off, old_read=capi.np_from(r.old_read, int(read_off[-1]), np.uint32), removed=capi.np_from(r.removed, int(so[-1]), np.uint8),
                      n_removed_snps=int(r.n_removed_snps), n_removed_cells=int(r.n_removed_cells), n_dropped_reads=int(r.n_dropped_reads),
                      new_first=capi.np_from(r.new_first, int(read_off[-1]), np.uint32), new_last=capi.np_from(r.new_last, int(read_off[-1]), np.uint32))
        load().floria_hip_mono_result_free(out)
        return ContigBatch(self, hs, n), result

    def mono_timing(self):
        """floria_hip_mono_timing: the device ms of the last drop_monomorphic call by kind"""
        ms = (C.c_double * 6)()
        _check(load().floria_hip_mono_timing(self._h, ms))
        return dict(zip(("clear_ms", "count_ms", "decide_ms", "filter_count_ms", "filter_fill_ms", "order_ms"), [float(x) for x in ms]))

    def haploset_alleles(self, contigs, grp_contig=None, groups=None, ranges=None, haplosets=None):
        """floria_hip_haploset_alleles: per haploset (read-id list + inclusive SNP range, as haploset_stats takes them) the number of its reads calling each allele
        at every SNP of its range -> (pos_off uint64 [n_groups + 1], counts uint32 [pos_off[-1], 4]): row pos_off[g] + (p - lo_g) is SNP p of group g."""
        if haplosets is not None:                    # the handle's groups; pos_off from the ranges of its download
            rg = haplosets.ranges().astype(np.int64)
            pos_off = np.zeros(len(rg) + 1, np.uint64)
            pos_off[1:] = np.cumsum(np.maximum(0, rg[:, 1] - rg[:, 0] + 1))
            counts = np.zeros((int(pos_off[-1]), 4), np.uint32)
            _check(load().floria_hip_haploset_alleles_resident(self._h, _contig_array(contigs), C.c_uint32(len(contigs)), haplosets._h, capi.ptr(pos_off, C.c_uint64),
                                                               capi.ptr(counts, C.c_uint32)))
            return pos_off, counts
        arr = (C.c_void_p * len(contigs))(*[c._h for c in contigs])
        gc = np.ascontiguousarray(grp_contig, np.uint32)
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups] + [np.zeros(0, np.uint32)]), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        lens = [max(0, int(hi) - int(lo) + 1) for lo, hi in np.asarray(ranges, np.int64).reshape(-1, 2)]
        pos_off = np.zeros(len(groups) + 1, np.uint64)
        pos_off[1:] = np.cumsum(lens)
        counts = np.zeros((int(pos_off[-1]), 4), np.uint32)
        _check(load().floria_hip_haploset_alleles(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64), capi.ptr(reads, C.c_uint32),
                                                  capi.ptr(rng, C.c_uint32), C.c_uint32(len(groups)), capi.ptr(pos_off, C.c_uint64), capi.ptr(counts, C.c_uint32)))
        return pos_off, counts

    def read_spans(self, contigs, grp_contig=None, groups=None, ranges=None, haplosets=None):
        """floria_hip_read_spans: per haploset (read-id list + inclusive SNP range, as haploset_alleles takes them; or groups = (grp_off, grp_read) arrays) and read the SEQ_POS word of the read's first
        cell with snp >= lo and of its last cell with snp <= hi -> (left uint32 [sum of the group sizes], right uint32 [same]); capi.FLORIA_SPAN_NONE where the
        read has no such cell.  Every contig must carry positions (assemble_contigs(keep_seq_pos=True), or drop_monomorphic of such contigs)."""
        n = len(contigs)
        arr = contigs._arr if isinstance(contigs, ContigBatch) else (C.c_void_p * max(n, 1))(*[c._h for c in contigs])
        if haplosets is not None:
            ne = haplosets.n_entries
            left = np.zeros(ne, np.uint32); right = np.zeros(ne, np.uint32)
            _check(load().floria_hip_read_spans_resident(self._h, arr, C.c_uint32(n), haplosets._h, capi.ptr(left, C.c_uint32), capi.ptr(right, C.c_uint32)))
            return left, right
        gc = np.ascontiguousarray(grp_contig, np.uint32)
        if isinstance(groups, tuple) and len(groups) == 2 and isinstance(groups[0], np.ndarray):      # (grp_off uint64 [n_groups + 1], grp_read uint32) as the C entry takes them
            off, reads = np.ascontiguousarray(groups[0], np.uint64), np.ascontiguousarray(groups[1], np.uint32)
        else:
            off = np.zeros(len(groups) + 1, np.uint64)
            off[1:] = np.cumsum([len(g) for g in groups])
            reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups] + [np.zeros(0, np.uint32)]), np.uint32)
        ng = len(off) - 1
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        if ng < 0 or len(gc) != ng or len(rng) != 2 * ng or (ng and len(reads) < int(off.max())):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "read_spans: one contig index and one (lo, hi) per group, grp_off[-1] read ids")
        left = np.zeros(int(off[-1]), np.uint32); right = np.zeros(int(off[-1]), np.uint32)
        _check(load().floria_hip_read_spans(self._h, arr, C.c_uint32(n), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64), capi.ptr(reads, C.c_uint32),
                                            capi.ptr(rng, C.c_uint32), C.c_uint32(ng), capi.ptr(left, C.c_uint32), capi.ptr(right, C.c_uint32)))
        return left, right

    def _pileup_records(self, blob, pos, flags, contig, cigar_off, n_cigar, seq_off, l_seq, qual_off, snp_off, snp_pos, alleles, n_alleles, refs=None, walk=None, resident=False):
        def arr(a, dt):
            return a if isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous else np.ascontiguousarray(a, dt)
        handle = blob if isinstance(blob, Blob) else None
        if handle is not None:
            if not resident:
                raise FloriaHipError(capi.FLORIA_E_INVALID, "pileup_records: a Blob handle is taken by pileup_records_resident alone")
            blob = np.zeros(0, np.uint8)
        keep = [arr(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, np.uint8), arr(pos, np.int32), arr(flags, np.uint16),
                arr(contig, np.uint32), arr(cigar_off, np.uint64), arr(n_cigar, np.uint32), arr(seq_off, np.uint64), arr(l_seq, np.uint32), arr(qual_off, np.uint64),
                arr(snp_off, np.uint64), arr(snp_pos, np.int64), arr(alleles, np.uint8), arr(n_alleles, np.uint8)]      # every input buffer stays alive until the call returns
        b, po, fl, ct, co, ncg, so, ls, qo, soff, sp, al, na = keep
        n = len(po)
        if not all(len(x) == n for x in (fl, ct, co, ncg, so, ls, qo)):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "pileup_records: the record arrays differ in length")
        if len(soff) < 1 or not (len(sp) == len(na) and al.size == 4 * len(sp)) or (len(soff) and int(soff[-1]) > len(sp)):
            raise FloriaHipError(capi.FLORIA_E_INVALID, "pileup_records: snp_off needs n_contigs + 1 entries, the last at most the number of SNPs; alleles is [n_snps, 4]")
        A = capi.CAlignments(capi.ptr(b, C.c_uint8), b.size, n, capi.ptr(po, C.c_int32), capi.ptr(fl, C.c_uint16), capi.ptr(ct, C.c_uint32), capi.ptr(co, C.c_uint64),
                             capi.ptr(ncg, C.c_uint32), capi.ptr(so, C.c_uint64), capi.ptr(ls, C.c_uint32), capi.ptr(qo, C.c_uint64))
        S = capi.CSnpTable(len(soff) - 1, capi.ptr(soff, C.c_uint64), capi.ptr(sp, C.c_int64), capi.ptr(al, C.c_uint8), capi.ptr(na, C.c_uint8))
        out = C.POINTER(capi.CRecordCells)()
        counts = None
        if resident:
            out = C.POINTER(capi.CRecordSummary)()
        if handle is not None:
            A.blob = None
            F = w = None
            if refs is not None:
                roff = arr(refs[0], np.uint64)
                rseq = arr(np.frombuffer(refs[1], np.uint8) if isinstance(refs[1], (bytes, bytearray, memoryview)) else (refs[1] if refs[1] is not None else []), np.uint8)
                keep += [roff, rseq]
                if len(roff) < 1 or (refs[1] is not None and int(roff.max()) > rseq.size):
                    raise FloriaHipError(capi.FLORIA_E_INVALID, "pileup_records_realign: ref_off needs n_contigs + 1 entries, the last at most len(ref_seq)")
                F = capi.CRefSeqs(len(roff) - 1, capi.ptr(roff, C.c_uint64), capi.ptr(rseq, C.c_uint8) if rseq.size else None)
                if walk is not None:
                    block, step, rule, tie = walk if len(walk) == 4 else (8,) + tuple(walk)
                    w = capi.CRealignWalk(int(block), int(step), {"max": 0, "sum": 1}.get(rule, rule), {"right": 0, "down": 1}.get(tie, tie))
            _check(load().floria_hip_pileup_records_resident_blob(self._h, handle._h, C.byref(A), C.byref(S), C.byref(F) if F is not None else None,
                                                                  C.byref(w) if w is not None else None, C.byref(out)))
            return RecordSummary(self, out, n)
        if refs is None and resident:
            _check(load().floria_hip_pileup_records_resident(self._h, C.byref(A), C.byref(S), None, None, C.byref(out)))
            return RecordSummary(self, out, n)
        if refs is None:
            _check(load().floria_hip_pileup_records(self._h, C.byref(A), C.byref(S), C.byref(out)))
        else:
            roff = arr(refs[0], np.uint64)
            rseq = arr(np.frombuffer(refs[1], np.uint8) if isinstance(refs[1], (bytes, bytearray, memoryview)) else (refs[1] if refs[1] is not None else []), np.uint8)
            keep += [roff, rseq]
            if len(roff) < 1 or (refs[1] is not None and int(roff.max()) > rseq.size):
                raise FloriaHipError(capi.FLORIA_E_INVALID, "pileup_records_realign: ref_off needs n_contigs + 1 entries, the last at most len(ref_seq)")
            F = capi.CRefSeqs(len(roff) - 1, capi.ptr(roff, C.c_uint64), capi.ptr(rseq, C.c_uint8) if rseq.size else None)
            w = None
            if walk is not None:
                block, step, rule, tie = walk if len(walk) == 4 else (8,) + tuple(walk)
                w = capi.CRealignWalk(int(block), int(step), {"max": 0, "sum": 1}.get(rule, rule), {"right": 0, "down": 1}.get(tie, tie))
            if resident:
                _check(load().floria_hip_pileup_records_resident(self._h, C.byref(A), C.byref(S), C.byref(F), C.byref(w) if w is not None else None, C.byref(out)))
                return RecordSummary(self, out, n)
            cc = capi.CRealignCounts()
            _check(load().floria_hip_pileup_records_realign(self._h, C.byref(A), C.byref(S), C.byref(F), C.byref(w) if w is not None else None, C.byref(out), C.byref(cc)))
            counts = dict(cells=int(cc.cells), in_bounds=int(cc.in_bounds), shortcut=int(cc.shortcut), scored=int(cc.scored), changed=int(cc.changed))
        r = out.contents
        cell_off = capi.np_from(r.cell_off, n + 1, np.uint64)
        t = int(cell_off[n])
        res = (cell_off, capi.np_from(r.snp, t, np.uint32), capi.np_from(r.allele, t, np.uint8), capi.np_from(r.qual, t, np.uint8),
               capi.np_from(r.seq_pos, t, np.uint32), capi.np_from(r.ref_end, n, np.int64))
        load().floria_hip_record_cells_free(out)
        del keep
        return res if refs is None else (res, counts)

    def hapq_batch(self, contigs, grp_contig=None, groups=None, ranges=None, snp_positions=None, block_length=None, haplosets=None):
        """get_hapq for the haplosets of many contigs in one call -> (hapq uint8 [n], rel_err float64 [n], avg_err float64 [n_contigs]).
        haplosets= a Haplosets handle made from `contigs`: its groups, nothing uploaded."""
        if haplosets is not None:
            pos = [np.ascontiguousarray(p, np.uint64) for p in snp_positions]
            pp = (C.POINTER(C.c_uint64) * max(1, len(pos)))(*[capi.ptr(p, C.c_uint64) for p in pos])
            ns = np.ascontiguousarray([len(p) for p in pos], np.uint32)
            ng = haplosets.n_groups
            hq = np.zeros(ng, np.uint8); rel = np.zeros(ng, np.float64); avg = np.zeros(len(contigs), np.float64)
            _check(load().floria_hip_hapq_batch_resident(self._h, _contig_array(contigs), C.c_uint32(len(contigs)), haplosets._h, pp, capi.ptr(ns, C.c_uint32),
                                                         C.c_uint64(int(block_length)), capi.ptr(hq, C.c_uint8), capi.ptr(rel, C.c_double), capi.ptr(avg, C.c_double)))
            return hq, rel, avg
        arr = (C.c_void_p * len(contigs))(*[c._h for c in contigs])
        gc = np.ascontiguousarray(grp_contig, np.uint32)
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if len(groups) else np.zeros(0, np.uint32), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        pos = [np.ascontiguousarray(p, np.uint64) for p in snp_positions]
        pp = (C.POINTER(C.c_uint64) * len(pos))(*[capi.ptr(p, C.c_uint64) for p in pos])
        ns = np.ascontiguousarray([len(p) for p in pos], np.uint32)
        hq = np.zeros(len(groups), np.uint8)
        rel = np.zeros(len(groups), np.float64)
        avg = np.zeros(len(contigs), np.float64)
        _check(load().floria_hip_hapq_batch(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64),
                                            capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32), C.c_uint32(len(groups)), pp, capi.ptr(ns, C.c_uint32),
                                            C.c_uint64(int(block_length)), capi.ptr(hq, C.c_uint8), capi.ptr(rel, C.c_double), capi.ptr(avg, C.c_double)))
        return hq, rel, avg

    # hap-graph paths -> haplosets on the resident S1 batch, and S2 from a handle ------------------------
    def join_paths(self, res, contigs, path_contig, nodes, ranges):
        """floria_hip_join_paths: path p of contig path_contig[p] (non-descending) is nodes[p], a sequence of (block, partition) of the S1 batch that produced `res`
        (still resident: the rule of hap_graph); ranges[p] = (lo, hi) is passed through -> Haplosets whose group p unites the nodes' reads."""
        off = np.zeros(len(nodes) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in nodes])
        flat = np.asarray([bk for n in nodes for bk in n], np.int64).reshape(-1, 2)
        return self.join_paths_raw(res, contigs, len(contigs), np.asarray(path_contig, np.uint32), off, flat[:, 0].astype(np.uint32), flat[:, 1].astype(np.uint8),
                                   np.asarray(ranges, np.uint32).reshape(-1), len(nodes))

    def join_paths_raw(self, res, contigs, n_contigs, path_contig, node_off, node_block, node_part, path_range, n_paths, token=None):
        """The C call with its arrays as given (None = NULL): what the refusal tests need."""
        def p(a, dt, ct):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dt)
            return a, capi.ptr(a, ct)
        keep = [p(path_contig, np.uint32, C.c_uint32), p(node_off, np.uint64, C.c_uint64), p(node_block, np.uint32, C.c_uint32), p(node_part, np.uint8, C.c_uint8),
                p(path_range, np.uint32, C.c_uint32)]
        cres = None
        if res is not None:
            bp = np.ascontiguousarray(res.best_ploidy, np.uint32)
            cres = capi.CBlockResult()
            cres.n_blocks = res.n_blocks; cres.max_ploidy = res.max_ploidy; cres.best_ploidy = capi.ptr(bp, C.c_uint32)
            cres.batch_token = res.batch_token if token is None else token
        h = C.c_void_p()
        _check(load().floria_hip_join_paths(self._h, C.byref(cres) if cres is not None else None, _contig_array(contigs) if contigs is not None else None, C.c_uint32(n_contigs),
                                            keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1], C.c_uint32(n_paths), C.byref(h)))
        return Haplosets(self, h, n_contigs)

    def reassign_haplosets_resident(self, contigs, haplosets, epsilon):
        """floria_hip_reassign_haplosets_resident: S2 whose input groups are a Haplosets handle (join_paths' or an earlier S2 call's) -> Haplosets; download() equals
        reassign_batch_resident on haplosets.download() with no read order.  `haplosets` is left as it is."""
        h = C.c_void_p()
        n = len(contigs) if contigs is not None else haplosets.n_contigs
        _check(load().floria_hip_reassign_haplosets_resident(self._h, _contig_array(contigs) if contigs is not None else None, C.c_uint32(n),
                                                             haplosets._h if haplosets is not None else None, C.c_double(epsilon), C.byref(h)))
        return Haplosets(self, h, n)

    # S2 --------------------------------------------------------------------------------------------
    def reassign_batch_resident(self, contigs, grp_contig, groups, ranges, epsilon, read_orders=None):
        """reassign_batch whose result stays on the device -> Haplosets (download() gives reassign_batch's list)."""
        return self.reassign_batch(contigs, grp_contig, groups, ranges, epsilon, read_orders, _resident=True)

    def reassign_batch(self, contigs, grp_contig, groups, ranges, epsilon, read_orders=None, _resident=False):
        """process_reads_for_final_parts for many resident contigs in one launch -> list of _capi.Groups (contig order)."""
        arr = _contig_array(contigs)
        gc = np.ascontiguousarray(grp_contig, np.uint32)
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if len(groups) else np.zeros(0, np.uint32), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        out = C.POINTER(C.POINTER(capi.CGroups))()
        if read_orders is None:
            po, poo = None, None
        else:                                        # one visiting order (array of read ids) per contig
            oo = np.zeros(len(contigs) + 1, np.uint64)
            oo[1:] = np.cumsum([len(o) for o in read_orders])
            ordv = np.ascontiguousarray(np.concatenate([np.asarray(o, np.uint32) for o in read_orders]) if len(read_orders) else np.zeros(0, np.uint32), np.uint32)
            po, poo = capi.ptr(ordv, C.c_uint32), capi.ptr(oo, C.c_uint64)
        if _resident:
            h = C.c_void_p()
            _check(load().floria_hip_reassign_batch_resident(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64),
                                                             capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32), C.c_uint32(len(groups)), po, poo,
                                                             C.c_double(epsilon), C.byref(h)))
            return Haplosets(self, h, len(contigs))
        _check(load().floria_hip_reassign_batch(self._h, arr, C.c_uint32(len(contigs)), capi.ptr(gc, C.c_uint32), capi.ptr(off, C.c_uint64),
                                                capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32), C.c_uint32(len(groups)), po, poo,
                                                C.c_double(epsilon), C.byref(out)))
        res = [capi.Groups(out[i].contents) for i in range(len(contigs))]
        load().floria_hip_groups_array_free(out, C.c_uint32(len(contigs)))
        return res

    def reassign(self, contig, groups, ranges, epsilon, read_order=None):
        """process_reads_for_final_parts (part_block_manip.rs:174-274): groups = list of read-id arrays,
        ranges = [(start,end)] -> _capi.Groups"""
        if isinstance(contig, Pileup):
            rc = self.upload(contig)
            try:
                return self.reassign(rc, groups, ranges, epsilon, read_order)
            finally:
                rc.free()
        off = np.zeros(len(groups) + 1, np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups])
        reads = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if len(groups) else np.zeros(0, np.uint32), np.uint32)
        rng = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        out = C.POINTER(capi.CGroups)()
        if read_order is None:
            po, no = None, 0
        else:
            ordv = np.ascontiguousarray(read_order, np.uint32)
            po, no = capi.ptr(ordv, C.c_uint32), len(ordv)
        _check(load().floria_hip_reassign_ordered(self._h, contig._h, capi.ptr(off, C.c_uint64), capi.ptr(reads, C.c_uint32), capi.ptr(rng, C.c_uint32),
                                                  C.c_uint32(len(groups)), po, C.c_uint32(no), C.c_double(epsilon), C.byref(out)))
        g = capi.Groups(out.contents)
        load().floria_hip_groups_free(out)
        return g
