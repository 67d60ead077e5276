"""`-m "not gpu"`: the decoder core of csrc/inflate_kernel.h — the text the GPU runs — compiled for the CPU as a stand-alone program (tests/cpp/inflate_core_check.cpp)
with -fsanitize=address,undefined and run as a program against zlib: every case of tests/inflate_cases.py, the named status for the malformed ones, then 2 000 seeded
single-bit and single-byte corruptions, each ending with some status or the right bytes inside the step bound 8 x payload + ISIZE, without a sanitizer report.  This
is the check that the malformed cases of tests/test_gpu_inflate.py are safe to send to a GPU.  And: the new symbols exist in the library and in the Python mirror."""
import os
import subprocess

from tests import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("floria_hip_inflate_bgzf", "floria_hip_blob_bytes", "floria_hip_blob_download", "floria_hip_blob_free", "floria_hip_blob_records",
               "floria_hip_blob_records_free", "floria_hip_pileup_records_resident_blob")


def test_decoder_core_against_zlib_under_the_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "inflate_core_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "inflate_core_check.cpp"), "-lz"], timeout=600)
    listed = ic.valid_cases() + ic.malformed_cases()
    assert len(listed) >= 25 and {s for _, _, _, s in listed} >= {0, 1, 2, 3, 4, 6, 7, 8}
    ic.write_case_file(cases, listed)
    r = subprocess.run([exe, cases, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all ok" in r.stdout and "2000 corruptions" in r.stdout and "FAILED" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    for name, _, _, _ in listed:
        assert name in r.stdout


def test_new_symbols_exist_in_the_library_and_the_mirror(hip_lib):
    L = hip_lib.load()
    for s in NEW_SYMBOLS:
        assert s in hip_lib.SYMBOLS and hasattr(L, s), s
    from floria_amd import _capi as capi
    assert hasattr(capi, "CBlobRecords") and hasattr(hip_lib, "Blob")
    for m in ("inflate_bgzf", "blob_records", "pileup_records_resident"):
        assert hasattr(hip_lib.FloriaHip, m)
