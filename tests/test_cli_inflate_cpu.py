"""`-m "not gpu"`: floria-hip --inflate host|device on the command line - the flag's refusals and its usage text, none of which needs a device - and what the route
rests on at the library boundary: floria_hip_blob_records_opt and floria_hip_blob_sequences exist in the library, the Python mirror and the Rust sketch, refuse
null arguments without a device, and the numpy model of the sequences (tests/blob_seq_model.py) is the two rules written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from floria_amd import _capi as capi
from tests import blob_seq_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "floria_amd", "host")

NEW_SYMBOLS = ("floria_hip_blob_records_opt", "floria_hip_blob_sequences", "floria_hip_blob_sequences_free")


@pytest.fixture(scope="module")
def floria_hip(hip_lib):
    subprocess.check_call(["make", "-C", HOST, "floria-hip"], stdout=subprocess.DEVNULL, timeout=900)
    return os.path.join(HOST, "floria-hip")


def run(floria_hip, *args):
    return subprocess.run([floria_hip, "-b", "none.bam", "-v", "none.vcf", "-r", "none.fa", *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("route", [(), ("--pileup", "host"), ("--pileup", "device"), ("--pileup", "fused")])
def test_inflate_device_without_pileup_resident_is_refused_with_the_reason(floria_hip, route):
    r = run(floria_hip, "--inflate", "device", *route)                   # (refused before any file is opened: the inputs do not exist)
    assert r.returncode == 1
    assert "--inflate device needs --pileup resident: only that route leaves the record bytes unread on the host" in r.stderr


def test_inflate_takes_host_or_device(floria_hip):
    r = run(floria_hip, "--inflate", "bogus")
    assert r.returncode == 1 and "--inflate takes host or device, not 'bogus'" in r.stderr
    r = run(floria_hip, "--inflate")
    assert r.returncode == 1 and "missing value for --inflate" in r.stderr
    # host is the default and is accepted on every route: the run gets as far as the BAM that is not there
    for extra in (("--inflate", "host"), ("--inflate", "host", "--pileup", "device")):
        r = run(floria_hip, *extra)
        assert r.returncode == 1 and "cannot open none.bam" in r.stderr and "--inflate" not in r.stderr


def test_help_names_the_flag(floria_hip):
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--inflate host|device" in r.stderr and "floria_hip_inflate_bgzf" in r.stderr and "Needs --pileup resident" in r.stderr


# ---- the library boundary the route rests on -------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_in_the_library_the_mirror_and_the_sketch(hip_lib):
    L = hip_lib.load()
    sketch = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW_SYMBOLS:
        assert s in hip_lib.SYMBOLS and hasattr(L, s) and "pub fn " + s + "(" in sketch, s
    assert capi.CBlobRecords._fields_[-1][0] == "chain_why" and "pub chain_why: *mut u32" in sketch      # appended: every earlier field keeps its place
    assert [f for f, _ in capi.CBlobSequences._fields_] == ["n", "base_off", "bases", "quals"] and "pub struct FloriaBlobSequences" in sketch
    header = open(os.path.join(ROOT, "include", "floria_hip.h")).read()
    assert f"#define FLORIA_CHAIN_CUT_TAIL {capi.FLORIA_CHAIN_CUT_TAIL}u" in header and f"#define FLORIA_CHAIN_ONE_REF  {capi.FLORIA_CHAIN_ONE_REF}u" in header
    assert hasattr(hip_lib.FloriaHip, "blob_sequences")


def test_null_arguments_are_refused_without_a_device(hip_lib):
    L = hip_lib.load()
    recs, seqs = C.POINTER(capi.CBlobRecords)(), C.POINTER(capi.CBlobSequences)()
    assert L.floria_hip_blob_records_opt(None, None, None, None, C.c_uint32(0), C.c_uint32(0), C.byref(recs)) == capi.FLORIA_E_INVALID
    assert b"null argument" in L.floria_hip_last_error() and not recs
    assert L.floria_hip_blob_sequences(None, None, None, None, None, C.c_uint64(0), C.byref(seqs)) == capi.FLORIA_E_INVALID
    assert b"null argument" in L.floria_hip_last_error() and not seqs
    L.floria_hip_blob_sequences_free(None)


def test_the_model_is_the_two_rules():
    assert bytes(model.bases([0x12, 0x48, 0xF0], 6)).decode() == "ACGTAA"
    assert bytes(model.bases([0x12, 0x48, 0xF0], 5)).decode() == "ACGTA" and len(model.bases([], 0)) == 0
    assert bytes(model.bases(np.arange(16, dtype=np.uint8), 32)[1::2]).decode() == "AACAGAAATAAAAAAA"        # the codes 0 .. 15 in the low nibble
    assert bytes(model.bases((np.arange(16) << 4).astype(np.uint8), 32)[0::2]).decode() == "AACAGAAATAAAAAAA"  # ... and in the high one
    assert model.quals([0, 1, 222, 223, 254, 255]).tolist() == [33, 34, 255, 255, 255, 255]
    raw = bytes([0xFF, 0x21, 0x80, 7, 8, 9, 0xFF])
    off, b, q = model.sequences(raw, [1, 1], [3, 2], [3, 4])
    assert off.tolist() == [0, 3, 5] and bytes(b).decode() == "CAT" + "CA" and q.tolist() == [40, 41, 42, 41, 42]
