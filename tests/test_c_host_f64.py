"""The host layer's double build: libdeciphon_host_f64.so, the four host sources compiled with -DIMM_DOUBLE_PRECISION
(imm_float = double), which a deciphon built with that macro links.

The C programs (tests/c/test_db_host_f64.c, tests/c/test_scan_host_f64.c) are compiled here with
-DIMM_DOUBLE_PRECISION and run as child processes: the two host libraries export the same names and are never loaded
into one process (the export lists are read with nm, not by loading).

CPU: both libraries build; the f64 one exports every function the header declares and the float one exports what it
exported before; a .dcp pressed in double round-trips bit for bit and says float_size 8; each build refuses the other's
file with the reference's code (src/db/reader.c:51, "invalid float size": RC_EINVAL); truncated and corrupted files
fail cleanly, also under ASan + UBSan; the reference's own test/protein_model.c passes in its double build.
GPU: the reference's test/protein_profile.c in its double build (hope's CLOSE then takes its double tolerance);
product rows of thread_run / thread_run_batch / scan_run_source against the C-ABI's; the LRT threshold in double;
imm_dp_viterbi after imm_dp_change_trans against the oracle's f64 recursion on the device's tables."""
import glob
import os
import subprocess

import numpy as np
import pytest

from test_c_host import HOST_DIR, LIBDIR, ROOT, build_c_test, build_host, declared_functions

HOST_F64_SO = os.path.join(LIBDIR, "libdeciphon_host_f64.so")
HOST_SO = os.path.join(LIBDIR, "libdeciphon_host.so")
OUT_F64 = os.path.join(ROOT, "oracle", "_ref", "compat_tests_f64")
RC_EINVAL = 3
F64_LIP = {"lip_write_f64", "lip_read_f64", "lip_write_1darray_f64_data", "lip_read_1darray_f64_data"}


def build_c_test_f64(tmp_path, name, extra=(), link_host=True):
    exe = str(tmp_path / name)
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DIMM_DOUBLE_PRECISION",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", name + ".c"), "-o", exe, "-L", LIBDIR]
    cmd += list(extra)
    cmd += (["-ldeciphon_host_f64"] if link_host else []) + ["-ldcp_hip", "-lm", "-fopenmp", "-Wl,-rpath," + LIBDIR]
    subprocess.check_call(cmd)
    return exe


def exported(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()[-2:-1] and line.split()[-2] in "TWDBR"}


def needed(path):
    out = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    return [line.split("[")[1].split("]")[0] for line in out.splitlines() if "(NEEDED)" in line]


def test_both_libraries_build_and_export_the_header(dcp, tmp_path):
    build_host()
    assert os.path.exists(HOST_SO) and os.path.exists(HOST_F64_SO)
    names = set(declared_functions())
    f32, f64 = exported(HOST_SO), exported(HOST_F64_SO)
    assert not names - f64, sorted(names - f64)
    assert not names - f32, sorted(names - f32)
    # one set of names in both; the double build adds its float64 MessagePack calls and nothing else, and the float
    # library does not grow by them
    assert f64 - f32 == F64_LIP and not f32 - f64
    assert not F64_LIP & f32
    # the scan test compiles against the header in double (it needs a GPU to run); what it links is the f64 library
    exe = build_c_test_f64(tmp_path, "test_scan_host_f64")
    assert "libdeciphon_host_f64.so" in needed(exe) and "libdeciphon_host.so" not in needed(exe)
    # and without the macro the double tests refuse to compile: nothing builds them against the wrong library
    src = os.path.join(ROOT, "tests", "c", "test_db_host_f64.c")
    r = subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "IMM_DOUBLE_PRECISION" in r.stderr


def test_db_host_f64_on_cpu(dcp, tmp_path):
    """sizeof(imm_float) == 8 (static assertions of the program), the .dcp round trip of every double with 1, 2 and 7
    partitions, the header's bytes, truncated and corrupted files"""
    build_host()
    exe = build_c_test_f64(tmp_path, "test_db_host_f64")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "all checks passed" in r.stdout


def test_each_build_refuses_the_other_s_file(dcp, tmp_path):
    build_host()
    exe64 = build_c_test_f64(tmp_path, "test_db_host_f64")
    tool32 = build_c_test(tmp_path, "dcp_tool")
    f32_db, f64_db = str(tmp_path / "f32.dcp"), str(tmp_path / "f64.dcp")
    subprocess.check_call([tool32, "press", f32_db, str(tmp_path / "side.bin"), "3", "40"])
    subprocess.check_call([exe64, "press", f64_db])
    raw32, raw64 = open(f32_db, "rb").read(), open(f64_db, "rb").read()
    assert raw32[raw32.index(b"float_size") + 10] == 4 and raw64[raw64.index(b"float_size") + 10] == 8
    # the double build's reader on a float file, and on its own
    r = subprocess.run([exe64, "open", f32_db], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith(f"rc={RC_EINVAL} RC_EINVAL"), r.stdout + r.stderr
    assert "float_size" in r.stderr
    r = subprocess.run([exe64, "open", f64_db], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("rc=0 "), r.stdout + r.stderr
    # the float build's reader on a double file, driven by the float test tool: protein_db_reader_open fails on
    # float_size before anything of a profile is read (no device call is reached).  Its code for float_size 8 is
    # RC_EINVAL: tests/c/test_db_host.c's header checks pin it.
    seqs = tmp_path / "seqs.txt"
    seqs.write_text("ACGT\n")
    r = subprocess.run([tool32, "scan", f64_db, str(seqs), str(tmp_path / "scores.bin"), "1", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "dcp_tool: reader open" in r.stderr and "float_size" in r.stderr, r.stderr


def test_db_host_f64_under_sanitizers(dcp, tmp_path):
    """The host layer's own C files compiled in double with ASan + UBSan (+ leak check) into the test: host code only."""
    srcs = sorted(glob.glob(os.path.join(HOST_DIR, "*.c")))
    exe = build_c_test_f64(tmp_path, "test_db_host_f64",
                           extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + srcs,
                           link_host=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "all checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def built_f64(name):
    exe = os.path.join(OUT_F64, name)
    if not os.path.exists(exe):
        pytest.skip(f"oracle/_ref/compat_tests_f64/{name} was not built (no reference tree at build time)")
    return exe


def test_reference_model_test_passes_in_its_double_build(dcp):
    exe = built_f64("protein_model")
    assert "libdeciphon_host_f64.so" in needed(exe) and "libdeciphon_host.so" not in needed(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_reference_protein_profile_test_passes_in_its_double_build_on_gpu():
    """goldens G1-G3 of test/protein_profile.c under hope's CLOSE for doubles (the reference's own macro)"""
    exe = built_f64("protein_profile")
    assert "libdeciphon_host_f64.so" in needed(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Assertion error" not in r.stderr


@pytest.mark.gpu
def test_c_scan_host_f64_on_gpu(tmp_path):
    build_host()
    exe = build_c_test_f64(tmp_path, "test_scan_host_f64")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "all checks passed" in r.stdout


def as_double(hexbits):
    return np.array([int(hexbits, 16)], np.uint64).view(np.float64)[0]


@pytest.mark.gpu
def test_viterbi_after_change_trans_is_the_oracle_s_f64_score(dcp, oracle64, tmp_path):
    """imm_dp_viterbi of the double build scores with the transitions the profile holds NOW: protein_profile_setup's,
    then four of them changed through imm_dp_change_trans.  Its null and alt logliks equal orc_dp_tables of the oracle's
    double build on the tables a double DB of the same sampled profile holds, with that row, as uint64.  (That the
    traced loglik equals the scanned one bitwise is imm_dp_viterbi's own return code, checked in the C program.)"""
    from test_f64_bits import Tables64

    build_host()
    exe = build_c_test_f64(tmp_path, "test_scan_host_f64")
    out = tmp_path / "viterbi.txt"
    r = subprocess.run([exe, "viterbi", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr[-3000:]
    lines = out.read_text().splitlines()
    assert len(lines) == 8
    sc = dcp.Scanner(0)
    changed = 0
    for line in lines:
        f = line.split()
        seed, M, entry, text = int(f[0]), int(f[1]), int(f[2]), f[3]
        eps = float(as_double(f[4]))
        xt = np.array([as_double(h) for h in f[5:18]])
        nul, alt = as_double(f[18]), as_double(f[19])
        prof = dcp.ProteinProfile.sample(seed, M, dcp.ProteinCfg(entry, eps), precision=64)
        assert prof.epsilon64 == eps
        sc.upload_db([prof])
        seq = dcp.encode_seq(text)
        sc.upload_seqs([seq])
        t8, em, ei, en = Tables64(sc, [prof]).t[0]
        rc, onl, oal = oracle64.dp_tables(t8, em, ei, en, xt, bytes(seq))
        assert rc == 0
        assert np.float64(nul).view(np.uint64) == np.float64(onl).view(np.uint64), (line, onl)
        assert np.float64(alt).view(np.uint64) == np.float64(oal).view(np.uint64), (line, oal)
        derived = [dcp.xtrans64(len(seq), mh, False) for mh in (True, False)]
        if not any(np.array_equal(xt.view(np.uint64), d.view(np.uint64)) for d in derived):
            changed += 1
            assert xt[10] == -1.7 and np.isfinite(xt[9])  # E -> J, E -> B as the program set them
    assert changed == 4
    sc.close()
