"""The packed cell of the optimise kernel's 4-byte stream (floria_amd/csrc/common.h: pk_pack / pk_delta / pk_allele / pk_qual, w24_table): a stand-alone C++
program (tests/cpp/packed_cell_test.cpp, its own main) built with -fsanitize=address,undefined round-trips the pack / unpack functions over the extremes and
checks the weight table against phred_scale.  Host code only: nothing here is loaded into Python, nothing needs a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_pack_unpack_round_trips_and_weight_table_under_sanitizers(tmp_path):
    # common.h is a HIP header, so the program goes through hipcc (the compiler the library itself needs); only its host side is instrumented and run
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "no hipcc: the library could not be built either"
    exe = str(tmp_path / "packed_cell_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "--offload-arch=gfx950",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "floria_amd", "csrc"), "-o", exe, os.path.join(CPP, "packed_cell_test.cpp")])
    syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "round trips, 256 weights: ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
