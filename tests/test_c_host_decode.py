"""scan_cfg.device_decode (include/deciphon_host.h): scan_run_source with the hits' paths decoded on the device, in the
float build of the host layer and in its double build.  tests/c/test_scan_decode.c is compiled against each library and
run as a child process (the two libraries export the same names and never share a process): the products of a job with
the switch set are those of a job without it, up to the codon of an M-state step whose two best codons tie."""
import subprocess

import pytest

from test_c_host import build_c_test, build_host
from test_c_host_f64 import build_c_test_f64, needed

BUILDS = {"float": (build_c_test, "libdeciphon_host.so"), "double": (build_c_test_f64, "libdeciphon_host_f64.so")}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_scan_decode_compiles_against_the_header(dcp, tmp_path, build):
    """CPU: the program builds with -Werror in either precision and links that precision's host library."""
    build_host()
    compile_test, lib = BUILDS[build]
    exe = compile_test(tmp_path, "test_scan_decode")
    assert lib in needed(exe) and len([n for n in needed(exe) if n.startswith("libdeciphon_host")]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_scan_decode_on_gpu(tmp_path, build):
    build_host()
    exe = BUILDS[build][0](tmp_path, "test_scan_decode")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
