"""scan_cfg.window / window_step / window_id (include/deciphon_host.h): scan_run_source over windows cut on the device, in
the float build of the host layer and in its double build.  tests/c/test_scan_windows.c is compiled against each library
and run as a child process (the two libraries export the same names and never share a process): the products of a job
with the members set are the bytes of a job whose source yields every window as a sequence of its own.

Also here: tests/c/asan_seq_windows.c, the three dcp_seq_window_* helpers under ASan + UBSan in a stand-alone CPU
program."""
import os
import subprocess

import pytest

from test_c_host import ROOT, build_c_test, build_host
from test_c_host_f64 import build_c_test_f64, needed

BUILDS = {"float": (build_c_test, "libdeciphon_host.so"), "double": (build_c_test_f64, "libdeciphon_host_f64.so")}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_scan_windows_compiles_against_the_header(dcp, tmp_path, build):
    """CPU: the program builds with -Werror in either precision and links that precision's host library."""
    build_host()
    compile_test, lib = BUILDS[build]
    exe = compile_test(tmp_path, "test_scan_windows")
    assert lib in needed(exe) and len([n for n in needed(exe) if n.startswith("libdeciphon_host")]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_scan_windows_on_gpu(tmp_path, build):
    build_host()
    exe = BUILDS[build][0](tmp_path, "test_scan_windows")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    assert "all checks passed" in r.stdout


def test_window_helpers_under_asan_ubsan(tmp_path):
    """CPU: dcp_seq_window_count / _start / _plan over the edge shapes, against the rule restated in the program, built
    with the host model alone (no device code) under ASan + UBSan."""
    obj, exe = str(tmp_path / "asan_seq_windows.o"), str(tmp_path / "asan_seq_windows")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_seq_windows.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_seq_windows ok" in r.stdout
