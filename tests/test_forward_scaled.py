"""The scaled probability-space Forward sweep: dcp_fwd_factor_f32, dcp_forward_scaled_tables (the host twin) and
dcp_gpu_forward_pairs_scaled / Scanner.forward_pairs_scaled (csrc/dcp_forward_scaled.h, .hip).

The reference is the log-space Forward the project already has: dcp_forward_tables on the host, forward_pairs on the
device.  -inf compares by equality; no NaN occurs anywhere.

The allowances:
  * device against the scaled host twin, either DB:            2^-32 (|x| + 1)
  * scaled host twin, double factors, against forward_tables:  2^-32 (|x| + 1)
  * scaled host twin, float factors, against forward_tables:   A = n(L, M) (delta + 2^-51), absolute, where delta is the
    factor rule's largest relative error over every float of its range (tests/c/fwd_factor_exhaustive.c, recorded in
    profiles/forward_scaled/factor_delta.txt) and n(L, M) = L (M + 2) + 2 counts the factors on the longest dependency
    chain behind the alt score: within a row one emission, the delete chain (MD and M - 2 DD), E -> B and the entry
    into the next row's P, at most M + 2; L rows; one factor at each end.  A sum of non-negative terms has at most its
    worst term's relative error, so every path's product is off by at most (1 + delta)^n and the log by n delta; 2^-51
    stands for the two double roundings beside each factor.  (DESIGN 24 has the derivation and the measured maxima.)

CPU: the factor rule sampled against math.exp and against the recorded delta; the host twin on test_forward_pairs'
     shapes; rescaling (700 nt, and a restatement in Python with band 4 and 64); the null state's own exponent; edge
     values; out of range; refusals; tests/c/asan_forward_scaled.c under ASan + UBSan as a program of its own.
GPU: per precision the device against the scaled host twin and against forward_pairs, on test_forward_pairs' world of
     class edges and test_forward_chain_edges' chain world; rescaling with small bands; few wavefronts; the redo list;
     lists, batches, refusals; everything else untouched."""
import ctypes as C
import ctypes.util
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import test_forward_chain_premises as pr
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, np_revcomp, refused
from test_forward_pairs import (CODE_OFF, FLAGS, NEG_INF, PRECISIONS, SHAPES, WORLD_L, WORLD_M, device_tables, oracle_case,
                                within, worst, xtrans_of)
from test_gpu_parity import pfam_like_params, planted_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MIN, T_MAX = np.float32(-708.0), np.float32(708.0)


def recorded_delta():
    with open(os.path.join(ROOT, "profiles", "forward_scaled", "factor_delta.txt")) as f:
        for line in f:
            if line.startswith("delta "):
                return float(line.split()[1])
    raise AssertionError("no delta recorded")


DELTA = recorded_delta()


def chain_factors(L, M):
    """n(L, M): the factors on the longest dependency chain behind the alt score (the docstring above)"""
    return L * (M + 2) + 2


def allowance_f32(L, M):
    return chain_factors(L, M) * (DELTA + 2.0 ** -51)


def within_f32(got, want, L, M):
    """the float factors' allowance, absolute; -inf by equality; never NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]) or np.isinf(got[~inf]).any():
        return False
    return bool(np.all(np.abs(got[~inf] - want[~inf]) <= allowance_f32(L, M)))


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32_of(b):
    return np.float32(struct.unpack("<f", struct.pack("<I", b))[0])


# ---- CPU: the factor rule -----------------------------------------------------------------------------------------
def test_factor_rule_sampled_against_exp(dcp):
    top = f32_bits(708.0)
    mags = set(range(0, top + 1, 257)) | {top}
    for e in range(0, (top >> 23) + 1):  # every binade's first and last float, the subnormals' too
        mags |= {max(e << 23, 0), min(((e + 1) << 23) - 1, top)}
    mags = sorted(m for m in mags if m <= top)
    worst_rel, prev = 0.0, None
    for sign in (0x80000000, 0):  # from -708 up to -0, then from +0 up to 708
        for m in (reversed(mags) if sign else mags):
            t = f32_of(m | sign)
            got, want = dcp.fwd_factor_f32(t), math.exp(float(t))
            assert got > 0.0 and math.isfinite(got)
            worst_rel = max(worst_rel, abs(got - want) / want)
            assert prev is None or got >= prev, (t, got, prev)  # monotone on the sample
            prev = got
    print("factor rule: sampled maximum %.4e, recorded delta %.4e" % (worst_rel, DELTA))
    assert 0.0 < worst_rel <= DELTA < 2.0 ** -23
    # the special values and the ends of the range, each within delta
    for t in (NEG_INF, -0.0, 0.0, T_MIN, T_MAX):
        got, want = dcp.fwd_factor_f32(t), (0.0 if t == NEG_INF else math.exp(float(t)))
        assert got == want or abs(got - want) <= DELTA * want, t
    assert dcp.fwd_factor_f32(NEG_INF) == 0.0 and dcp.fwd_factor_f32(0.0) == 1.0 and dcp.fwd_factor_f32(-0.0) == 1.0
    assert dcp.fwd_factor_f32(np.nextafter(T_MIN, np.float32(-np.inf))) == 0.0 and dcp.fwd_factor_f32(-1e30) == 0.0
    assert dcp.fwd_factor_f32(T_MIN) >= 2.2250738585072014e-308  # still a normal double
    assert dcp.fwd_factor_f32(np.nextafter(T_MAX, np.float32(np.inf))) == math.inf
    for t in (0.4, 0.7, 3.0, 88.0, 100.0, 700.0):  # positive t: positive MD / DD, and beyond float's own range
        assert abs(dcp.fwd_factor_f32(t) / math.exp(float(np.float32(t))) - 1.0) <= DELTA


def test_factor_rule_exhaustive_program_builds_and_its_record_is_there(tmp_path):
    """the program itself runs once, by hand (2.3e9 floats); here: it compiles, and what it printed is committed"""
    obj = str(tmp_path / "fwd_factor_exhaustive.o")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "fwd_factor_exhaustive.c"), "-o", obj])
    text = open(os.path.join(ROOT, "profiles", "forward_scaled", "factor_delta.txt")).read()
    assert "floats 2288123906" in text and "ends ok" in text and "steps against the direction of exp 0" in text


# ---- CPU: the host twin -------------------------------------------------------------------------------------------
def scaled(dcp, tabs, xt, seq, f32=False, band=None):
    n, a, oor = dcp.forward_scaled_tables(*tabs, xt, seq, float_factors=f32, band=band)
    assert not oor
    return n, a


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_with_double_factors(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):  # float tables go in promoted
        t8, em, ei, en, xt, seq = oracle_case(orc, M, L, multi)
        want = dcp.forward_tables(t8, em, ei, en, xt, seq)
        got = scaled(dcp, (t8, em, ei, en), xt, seq)
        print("scaled twin, double factors, vs forward_tables M %d L %d multi %d f%d: %.3e" % (
            M, L, multi, 64 if orc is oracle64 else 32, worst(got, want)))
        assert within(got, want), (got, want)
        if L == 1:  # one word, one path through R: the Viterbi bits, within the allowance
            rc, vn, va = orc.dp_tables(t8, em, ei, en, xt, bytes(seq))
            assert rc == 0 and within([got[0]], [float(vn)])


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_with_float_factors(dcp, oracle32, M, L, multi):
    t8, em, ei, en, xt, seq = oracle_case(oracle32, M, L, multi)
    want = dcp.forward_tables(t8, em, ei, en, xt, seq)
    got = scaled(dcp, (t8, em, ei, en), xt, seq, f32=True)
    d = max(abs(got[0] - want[0]), abs(got[1] - want[1]))
    print("scaled twin, float factors, vs forward_tables M %d L %d multi %d: |d| %.3e, A = %d x %.3e = %.3e" % (
        M, L, multi, d, chain_factors(L, M), DELTA, allowance_f32(L, M)))
    assert within_f32(got, want, L, M), (got, want)
    assert got != scaled(dcp, (t8, em, ei, en), xt, seq)  # the float rule is in use


_LIBM = C.CDLL(ctypes.util.find_library("m"))
_LIBM.fma.restype, _LIBM.fma.argtypes = C.c_double, [C.c_double] * 3
fma = _LIBM.fma


def exp_or_inf(t):
    """exp in double as the C library rounds it: 0 for -inf, +inf past the range (math.exp raises there)"""
    try:
        return math.exp(t) if t != NEG_INF else 0.0
    except OverflowError:
        return math.inf


def restate_scaled(t8, em, ei, en, xt, seq, band, where=False):
    """dcp_forward_scaled.h's rule with double factors, in Python: (null, alt, s, sR).

    where: also where the rule ends the pair, by the twin's checks in the twin's order -- row 0's P and PN; per row P,
    Q, E, B, PN, PJ, PC, PR; then alt.  Returns (null, alt, s, sR, exit, names): exit is None for a pair that stays in
    range, ("row", j) for a non-finite value in row j, ("finish",) for a non-finite alt, the scores are None with an
    exit, s and sR are the exponents reached by then, and names are the row's non-finite values in the order checked."""
    f = exp_or_inf
    fin = math.isfinite
    T = [[f(float(v)) for v in row] for row in np.asarray(t8, np.float64)]
    ENT, MM, IM, DM, MD, DD, MI, II = T
    RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB = (f(float(v)) for v in xt)
    em, ei, en = np.asarray(em, np.float64), np.asarray(ei, np.float64), np.asarray(en, np.float64)
    M, L = len(ENT), len(seq)
    P, Q = [[0.0] * M for _ in range(5)], [[0.0] * M for _ in range(5)]
    PN, PJ, PC, PR = [0.0] * 5, [0.0] * 5, [0.0] * 5, [0.0] * 5
    s = sR = 0
    w, E, Cc, Rr = 0, 0.0, 0.0, 0.0

    def step_of(ref, band=band):
        if ref == 0.0:
            return 0
        k = max((struct.unpack("<Q", struct.pack("<d", ref))[0] >> 52) & 0x7FF, 1) - 1023
        return 0 if -band <= k < band else min(k, 1022)

    B0, PN[0], PR[0] = SB, SN, 1.0
    if fin(B0) and fin(PN[0]):  # row 0 is a row: ref = max(PN, B), before P is formed
        s = step_of(max(PN[0], B0))
        B0, PN[0] = B0 * 2.0 ** -s, PN[0] * 2.0 ** -s
    P[0] = [B0 * e for e in ENT]
    names = (["P"] if not all(fin(v) for v in P[0]) else []) + (["PN"] if not fin(PN[0]) else [])
    if where and names:
        return None, None, s, sR, ("row", 0), names

    for j in range(1, L + 1):
        w = ((w << 2) | int(seq[j - 1])) & 1023
        code = [CODE_OFF[l] + (w & ((1 << (2 * (l + 1))) - 1)) for l in range(5)]
        slot = [(j + 4 - l) % 5 for l in range(5)]
        fN, fI = [f(float(en[c])) for c in code], [f(float(ei[c])) for c in code]
        fM = [[f(float(v)) for v in em[c]] for c in code]
        N = J = Cc = Rr = 0.0
        for l in range(5):
            N, J = fma(PN[slot[l]], fN[l], N), fma(PJ[slot[l]], fN[l], J)
            Cc, Rr = fma(PC[slot[l]], fN[l], Cc), fma(PR[slot[l]], fN[l], Rr)
        Mr, Ir, Dr = [0.0] * M, [0.0] * M, [0.0] * M
        for k in range(M):
            for l in range(5):
                Mr[k] = fma(P[slot[l]][k], fM[l][k], Mr[k])
                Ir[k] = fma(Q[slot[l]][k], fI[l], Ir[k])
        for k in range(1, M):
            Dr[k] = fma(DD[k], Dr[k - 1], Mr[k - 1] * MD[k])
        E = 0.0
        for k in range(M):
            E += Mr[k]
            if k:
                E += Dr[k]
        B = fma(J, JB, fma(E, EB, N * NB))
        r = j % 5
        for k in range(M):
            p = B * ENT[k]
            if k:
                p = fma(Dr[k - 1], DM[k], fma(Ir[k - 1], IM[k], fma(Mr[k - 1], MM[k], p)))
            P[r][k], Q[r][k] = p, fma(Ir[k], II[k], Mr[k] * MI[k])
        PN[r], PJ[r], PC[r], PR[r] = N * NN, fma(J, JJ, E * EJ), fma(Cc, CC, E * EC), Rr * RR
        if where:
            checked = (("P", P[r]), ("Q", Q[r]), ("E", [E]), ("B", [B]), ("PN", [PN[r]]), ("PJ", [PJ[r]]), ("PC", [PC[r]]),
                       ("PR", [PR[r]]))
            names = [name for name, vals in checked if not all(fin(v) for v in vals)]
            if names:
                return None, None, s, sR, ("row", j), names
        k = step_of(max(PN[r], PJ[r], PC[r], E, B))
        if k:
            c = 2.0 ** -k
            P, Q = [[v * c for v in row] for row in P], [[v * c for v in row] for row in Q]
            PN, PJ, PC = [v * c for v in PN], [v * c for v in PJ], [v * c for v in PC]
            E, Cc, s = E * c, Cc * c, s + k
        k = step_of(PR[r])
        if k:
            PR, Rr, sR = [v * 2.0 ** -k for v in PR], Rr * 2.0 ** -k, sR + k

    def score(u, s):
        if u == 0.0:
            return NEG_INF
        m, e = math.frexp(u)
        return math.log(m) + float(e + s) * 0.693147180559945309417232121458

    k = step_of(max(E, Cc), 0) if fin(E) and fin(Cc) else 0  # the finish: the larger of E and C into [1, 2), whatever the band
    alt = fma(Cc * 2.0 ** -k, CT, (E * 2.0 ** -k) * ET)  # (s, as returned, is the rows' exponent: where the band left it)
    if not where:
        return score(Rr, sR), score(alt, s + k), s, sR
    if not fin(alt):
        return None, None, s, sR, ("finish",), ["alt"]
    return score(Rr, sR), score(alt, s + k), s, sR, None, []


@pytest.mark.parametrize("M", [2, 40])
def test_rescaling_700_nt(dcp, oracle64, M):
    L = 700
    t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
    want = dcp.forward_tables(t8, em, ei, en, xt, seq)
    assert math.exp(want[0]) == 0.0 and want[0] < -745.0  # the premise: unscaled, the null path alone underflows double
    got = scaled(dcp, (t8, em, ei, en), xt, seq)
    assert np.isfinite(got).all() and within(got, want)
    assert within_f32(scaled(dcp, (t8, em, ei, en), xt, seq, f32=True), dcp.forward_tables(t8, em, ei, en, xt, seq), L, M)
    steps = set()
    for band in (4, 64):
        rn, ra, s, sR = restate_scaled(t8, em, ei, en, xt, seq, band)
        assert s < -1000 and sR < -1000  # both exponents moved
        steps.add((s, sR))
        assert bits(np.array([rn, ra])).tolist() == bits(np.array(got)).tolist(), band  # the twin's bits both times
        assert scaled(dcp, (t8, em, ei, en), xt, seq, band=band) == got
    assert len(steps) == 2  # the two bands rescaled at different rows


def planted_case(orc, multi=True):
    """a 300-node profile's own gene between flanks: 1 000 nt (the pair of tests/test_scan_pairs.py's kind)"""
    rng = np.random.default_rng(1764)
    params = pfam_like_params(rng, 300)
    gene = planted_query(rng, orc.new(*params, ENTRY_DIST_OCCUPANCY, 0.01), 300, flank=50)
    p = orc.new(*params, ENTRY_DIST_OCCUPANCY, 0.01)
    p.setup(len(gene), multi, False)
    return p.export() + (gene,)


def test_the_null_state_keeps_its_own_exponent(dcp, oracle64, oracle32):
    for orc in (oracle64, oracle32):
        t8, em, ei, en, xt, seq = planted_case(orc)
        want = dcp.forward_tables(t8, em, ei, en, xt, seq)
        assert want[1] - want[0] > 750.0, want  # a condition on the input: one exponent for both would flush R to zero
        got = scaled(dcp, (t8, em, ei, en), xt, seq)
        assert np.isfinite(got).all() and within(got, want), (got, want)
        if orc is oracle32:
            gf = scaled(dcp, (t8, em, ei, en), xt, seq, f32=True)
            assert np.isfinite(gf).all() and within_f32(gf, want, len(seq), 300)


def test_edge_values(dcp, oracle64):
    for L in (1, 7, 10):  # epsilon = 0 and L mod 3 != 0: no path, -inf twice (ref == 0 rescales nothing)
        t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, L, True, eps=0.0)
        for f32 in (False, True):
            assert dcp.forward_scaled_tables(t8, em, ei, en, xt, seq, float_factors=f32) == (NEG_INF, NEG_INF, False)
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 9, True, eps=0.0)
    assert within(scaled(dcp, (t8, em, ei, en), xt, seq), dcp.forward_tables(t8, em, ei, en, xt, seq))
    for M, L in ((2, 7), (5, 30), (65, 60)):  # ldk > M: the bits of ldk = M
        t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
        ldk = M + 7
        t8p, emp = np.full((8, ldk), 3.0), np.full((1364, ldk), 3.0)  # padding the twin must never read as a column
        t8p[:, :M], emp[:, :M] = t8, em
        null, alt, oor = C.c_double(1.0), C.c_double(2.0), C.c_int(7)
        rc = dcp.lib.dcp_forward_scaled_tables(M, ldk, t8p.ctypes.data, emp.ctypes.data, ei.ctypes.data, en.ctypes.data,
                                               xt.ctypes.data, seq.ctypes.data, L, 0, C.byref(null), C.byref(alt), C.byref(oor))
        assert rc == 0 and oor.value == 0
        want = scaled(dcp, (t8, em, ei, en), xt, seq)
        assert bits(np.array([null.value, alt.value])).tolist() == bits(np.array(want)).tolist()


def test_out_of_range_is_flagged_and_writes_nothing(dcp, oracle64):
    M, L = 2000, 12
    t8, em, ei, en, xt, seq = pr.tables(oracle64, "positive", M, L)
    assert float(np.sum(t8[5, 1:])) > 720.0  # the sum of DD: the chain multiplies up past the double range
    want = dcp.forward_tables(t8, em, ei, en, xt, seq)
    assert np.isfinite(want).all()
    for f32 in (False, True):
        null, alt, oor = C.c_double(1.5), C.c_double(2.5), C.c_int(0)
        rc = dcp.lib.dcp_forward_scaled_tables(M, M, t8.ctypes.data, em.ctypes.data, ei.ctypes.data, en.ctypes.data, xt.ctypes.data,
                                               seq.ctypes.data, L, int(f32), C.byref(null), C.byref(alt), C.byref(oor))
        assert rc == 0 and oor.value == 1 and (null.value, alt.value) == (1.5, 2.5)  # no NaN, no +inf: nothing at all
        assert dcp.forward_scaled_tables(t8, em, ei, en, xt, seq, float_factors=f32) == (None, None, True)
    # the positive chain of 600 nodes stays in range
    t8, em, ei, en, xt, seq = pr.tables(oracle64, "positive", 600, 12)
    assert within(scaled(dcp, (t8, em, ei, en), xt, seq), dcp.forward_tables(t8, em, ei, en, xt, seq))


def test_host_twin_refusals(dcp, oracle64):
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    P = lambda a: a.ctypes.data  # noqa: E731
    good = dict(M=5, ldk=5, t8=P(t8), em=P(em), ei=P(ei), en=P(en), xt=P(xt), seq=P(seq), L=30)
    bad_seq = seq.copy()
    bad_seq[17] = 4
    wide = np.full((8, 4097), NEG_INF), np.full((1364, 4097), NEG_INF)
    cases = [dict(M=0), dict(M=4097, ldk=4097, t8=P(wide[0]), em=P(wide[1])), dict(ldk=4), dict(L=0), dict(seq=P(bad_seq)),
             dict(t8=None), dict(em=None), dict(ei=None), dict(en=None), dict(xt=None), dict(seq=None)]
    for change in cases:
        a = dict(good, **change)
        null, alt, oor = C.c_double(1.5), C.c_double(2.5), C.c_int(7)
        rc = dcp.lib.dcp_forward_scaled_tables(a["M"], a["ldk"], a["t8"], a["em"], a["ei"], a["en"], a["xt"], a["seq"], a["L"], 0,
                                               C.byref(null), C.byref(alt), C.byref(oor))
        assert rc == dcp.RC_EINVAL and (null.value, alt.value, oor.value) == (1.5, 2.5, 7), change
    null, oor = C.c_double(1.5), C.c_int(7)
    for outs in ((None, C.byref(null), C.byref(oor)), (C.byref(null), None, C.byref(oor)), (C.byref(null), C.byref(null), None)):
        assert dcp.lib.dcp_forward_scaled_tables(5, 5, P(t8), P(em), P(ei), P(en), P(xt), P(seq), 30, 0, *outs) == dcp.RC_EINVAL
        assert null.value == 1.5 and oor.value == 7
    for band in (0, 501, -1):
        assert dcp.lib.dcp_forward_scaled_tables_band(5, 5, P(t8), P(em), P(ei), P(en), P(xt), P(seq), 30, 0, band, C.byref(null),
                                                      C.byref(null), C.byref(oor)) == dcp.RC_EINVAL
    with pytest.raises(dcp.DcpError):
        dcp.forward_scaled_tables(t8, em[:, :4], ei, en, xt, seq)


def test_forward_scaled_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_forward_scaled.c with the host model alone (no device code) under ASan + UBSan, as a program
    of its own."""
    obj, exe = str(tmp_path / "asan_forward_scaled.o"), str(tmp_path / "asan_forward_scaled")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_forward_scaled.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_forward_scaled ok" in r.stdout


# ---- GPU ------------------------------------------------------------------------------------------------------------
import test_forward_chain_edges as ce  # noqa: E402
import test_forward_pairs as fp  # noqa: E402

_TWIN = {}


def scaled_twin_of(dcp, precision, tabs, seqs, key):
    """per flags the scaled host twin's (null, alt, out_of_range) matrices on the tables the device holds"""
    if key not in _TWIN:
        out = {}
        for multi, h3 in FLAGS:
            n, a = np.zeros((len(seqs), len(tabs))), np.zeros((len(seqs), len(tabs)))
            oor = np.zeros((len(seqs), len(tabs)), bool)
            for q, s in enumerate(seqs):
                xt = xtrans_of(dcp, precision, len(s), multi, h3)
                for p in range(len(tabs)):
                    gn, ga, flag = dcp.forward_scaled_tables(*tabs[p], xt, s, float_factors=precision == 32)
                    oor[q, p] = flag
                    n[q, p], a[q, p] = (np.nan, np.nan) if flag else (gn, ga)
            out[multi, h3] = (n, a, oor)
            if key[0] == "chain":
                break  # the chain world runs multi-hit alone
        _TWIN[key] = out
    return _TWIN[key]


def check_against_the_reference(precision, got, ref, sq, pp, seqs, profs):
    """forward_pairs of the same list, at the allowance of the DB kind"""
    for g, w in zip(got, ref):
        assert np.array_equal(np.isfinite(g), np.isfinite(w))  # finite exactly where forward_pairs is
        if precision == 64:
            assert within(g, w)
        else:
            for i in range(len(sq)):
                assert within_f32(g[i:i + 1], w[i:i + 1], len(seqs[sq[i]]), profs[pp[i]].core_size), (i, g[i], w[i])


def shuffled(nq, npf, seed):
    every = [(q, p) for q in range(nq) for p in range(npf)]
    order = np.random.default_rng(seed).permutation(len(every))
    return np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_class_edges_against_the_twin_and_forward_pairs(dcp, oracle64, precision, multi, h3):
    profs, seqs, tabs = fp.world(dcp, precision, oracle64)[:3]
    tn, ta, oor = scaled_twin_of(dcp, precision, tabs, seqs, ("edges", precision))[multi, h3]
    assert not oor.any()
    sq, pp = shuffled(len(seqs), len(profs), 17)
    sc = fp.loaded(dcp, precision)
    assert sc.forward_scaled_kernel_ms < 0
    gn, ga = sc.forward_pairs_scaled(sq, pp, multi, h3)
    assert sc.forward_scaled_kernel_ms > 0 and sc.last_forward_scaled_redo_pairs == 0
    ref = sc.forward_pairs(sq, pp, multi, h3)
    sc.close()
    print("scaled device vs scaled twin f%d multi %d h3 %d: null %.3e alt %.3e; vs forward_pairs: |d| null %.3e alt %.3e" % (
        precision, multi, h3, worst(gn, tn[sq, pp]), worst(ga, ta[sq, pp]),
        np.nanmax(np.abs(np.where(np.isfinite(ref[0]), gn - ref[0], 0.0))), np.nanmax(np.abs(np.where(np.isfinite(ref[1]), ga - ref[1], 0.0)))))
    assert within(gn, tn[sq, pp]) and within(ga, ta[sq, pp])
    check_against_the_reference(precision, (gn, ga), ref, sq, pp, seqs, profs)
    assert np.isfinite(ga).sum() > len(sq) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_delete_chain_and_chunks(dcp, precision):
    specs, profs, seqs = ce.chain_world(dcp, precision)[:3]
    sc = ce.loaded(dcp, precision)
    tabs = device_tables(dcp, sc, profs, precision, pr.EPS)
    if precision == 32:
        for p, (fam, M, k, eps) in enumerate(specs):
            if eps != pr.EPS:
                tabs[p] = tabs[p][:2] + (dcp.frame_table_host(profs[p].insert_dist, eps), dcp.frame_table_host(profs[p].null_dist, eps))
    tn, ta, oor = scaled_twin_of(dcp, precision, tabs, seqs, ("chain", precision))[True, False]
    assert not oor.any()
    sq, pp = shuffled(len(seqs), len(profs), 13)
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    assert sc.last_forward_scaled_redo_pairs == 0
    ref = sc.forward_pairs(sq, pp)
    sc.close()
    fam = np.array([specs[p][0] for p in pp])
    for f in ce.FAMILIES:
        ix = np.nonzero(fam == f)[0]
        print("scaled device vs scaled twin f%d %s, %d pairs: null %.3e alt %.3e" % (
            precision, f, len(ix), worst(gn[ix], tn[sq[ix], pp[ix]]), worst(ga[ix], ta[sq[ix], pp[ix]])))
        assert within(gn[ix], tn[sq[ix], pp[ix]]) and within(ga[ix], ta[sq[ix], pp[ix]]), f
    check_against_the_reference(precision, (gn, ga), ref, sq, pp, seqs, profs)
    eps0 = np.array([specs[p][0] == "eps0" and len(seqs[q]) % 3 != 0 for q, p in zip(sq, pp)])
    assert (gn[eps0] == NEG_INF).all() and (ga[eps0] == NEG_INF).all() and np.isfinite(ga[~eps0]).all()


def planted_pair_world(dcp, orc, precision):
    """the 300-node profile and its planted 1 000-nt query, the world's profiles of 1, 64, 65 and 257 nodes, a 700-nt
    query"""
    rng = np.random.default_rng(1764)
    params = pfam_like_params(rng, 300)
    gene = planted_query(rng, orc.new(*params, ENTRY_DIST_OCCUPANCY, 0.01), 300, flank=50)
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
    planted = dcp.ProteinProfile.from_params(*params, cfg, "PLANTED", precision=precision)
    long = np.random.default_rng(700).integers(0, 4, 700, dtype=np.uint8)
    return planted, gene, long


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rescaling_on_the_device(dcp, oracle64, oracle32, precision):
    profs, seqs, tabs = fp.world(dcp, precision, oracle64)[:3]
    planted, gene, long = planted_pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    ix = [WORLD_M.index(M) for M in (1, 64, 65, 257)]
    mine = [profs[i] for i in ix] + [planted]
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(mine)
    sc.upload_seqs([long, gene])
    mytabs = device_tables(dcp, sc, mine, precision, float(np.float32(0.01)))
    sq, pp = np.array([0, 0, 0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 3, 4, 4, 3, 0])
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    ref = sc.forward_pairs(sq, pp)
    assert ref[1][5] - ref[0][5] > 750.0  # the planted pair: a condition on the input
    assert np.isfinite(gn).all() and np.isfinite(ga).all() and sc.last_forward_scaled_redo_pairs == 0
    assert (gn < -745.0).all()  # unscaled, every null path would underflow double
    for i, (q, p) in enumerate(zip(sq, pp)):
        s = (long, gene)[q]
        tw = dcp.forward_scaled_tables(*mytabs[p], xtrans_of(dcp, precision, len(s), True, False), s, float_factors=precision == 32)
        assert not tw[2] and within([gn[i]], [tw[0]]) and within([ga[i]], [tw[1]]), (i, gn[i], ga[i], tw)
    check_against_the_reference(precision, (gn, ga), ref, sq, pp, (long, gene), mine)
    for band in (4, 8):
        sc.test_set_forward_scale_band(band)
        g2 = sc.forward_pairs_scaled(sq, pp)
        assert np.array_equal(bits(g2[0]), bits(gn)) and np.array_equal(bits(g2[1]), bits(ga)), band
    sc.test_set_forward_scale_band(0)
    # the whole first world again with small bands: the same bits as the default, the wide class's work-area rings too
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sq, pp = shuffled(len(seqs), len(profs), 17)
    base = {f: sc.forward_pairs_scaled(sq, pp, *f) for f in FLAGS}
    for band in (4, 8):
        sc.test_set_forward_scale_band(band)
        for f in FLAGS:
            got = sc.forward_pairs_scaled(sq, pp, *f)
            assert np.array_equal(bits(got[0]), bits(base[f][0])) and np.array_equal(bits(got[1]), bits(base[f][1])), (band, f)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_launches(dcp, oracle64, precision):
    profs, seqs = fp.world(dcp, precision, oracle64)[:2]
    ix = {M: i for i, M in enumerate(WORLD_M)}
    q = WORLD_L.index(100)
    pairs = [(q, ix[1100]), (q, ix[257]), (q, ix[1100]), (q, ix[2]), (q, ix[513])]
    pairs += [(8, ix[512]), (7, ix[64]), (8, ix[129]), (5, ix[1100]), (8, len(WORLD_M)), (6, ix[256])]
    sq, pp = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    sc = fp.loaded(dcp, precision, dcp.load_testhooks())
    base = sc.forward_pairs_scaled(sq, pp)
    for cap in (3, 1, 0):
        sc.test_set_forward_waves(cap)
        got = sc.forward_pairs_scaled(sq, pp)
        assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1])), cap
    sc.close()
    # a 4 096-node, a 257-node, a severed 1 100-node and a 64-node pair behind one another, twice
    specs = ce.chain_world(dcp, precision)[0]
    at = [ce.index_of(specs, "delete", 4096), ce.index_of(specs, "delete", 257), ce.index_of(specs, "severed", 1100, 512),
          ce.index_of(specs, "delete", 64)]
    sq, pp = np.array([3, 2, 3, 1] * 2), np.array(at * 2)
    sc = ce.loaded(dcp, precision, dcp.load_testhooks())
    base = sc.forward_pairs_scaled(sq, pp)
    assert np.isfinite(base[1]).all() and np.array_equal(bits(base[1][:4]), bits(base[1][4:]))
    for cap in (1, 3):
        sc.test_set_forward_waves(cap)
        got = sc.forward_pairs_scaled(sq, pp)
        assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1])), cap
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_redo_of_pairs_out_of_range(dcp, oracle64, precision):
    profs, seqs = fp.world(dcp, precision, oracle64)[:2]
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
    big = dcp.ProteinProfile.from_params(*pr.chain_params("positive", 2000), cfg, "POS2000", precision=precision)
    keep = [WORLD_M.index(M) for M in (2, 64, 129, 256, 513)]
    mine = [profs[i] for i in keep[:3]] + [big] + [profs[i] for i in keep[3:]]
    qs = [WORLD_L.index(L) for L in (6, 17, 100)]
    sc = dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs([seqs[q] for q in qs])
    sq, pp = shuffled(3, len(mine), 5)
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    flagged = pp == 3
    assert sc.last_forward_scaled_redo_pairs == int(flagged.sum()) == 3
    ref = sc.forward_pairs(sq, pp)
    assert np.isfinite(ref[1][flagged]).all() and not np.isnan(ga).any() and not np.isnan(gn).any()
    # its pairs return forward_pairs' bits ...
    assert np.array_equal(bits(gn[flagged]), bits(ref[0][flagged])) and np.array_equal(bits(ga[flagged]), bits(ref[1][flagged]))
    # ... and the other pairs' bits are the same as without it in the list
    on, oa = sc.forward_pairs_scaled(sq[~flagged], pp[~flagged])
    assert sc.last_forward_scaled_redo_pairs == 0
    assert np.array_equal(bits(on), bits(gn[~flagged])) and np.array_equal(bits(oa), bits(ga[~flagged]))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lists_batches_and_refusals(dcp, oracle64, precision):
    profs, seqs, tabs = fp.world(dcp, precision, oracle64)[:3]
    f32 = precision == 32

    def twin(p, xt, s):
        n, a, oor = dcp.forward_scaled_tables(*tabs[p], xt, s, float_factors=f32)
        assert not oor
        return n, a

    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.forward_pairs_scaled([0], [0]))  # no DB
    sc.upload_db(profs)
    refused(dcp, sc, lambda: sc.forward_pairs_scaled([0], [0]))  # no batch
    sc.upload_seqs(seqs)
    assert sc.forward_scaled_kernel_ms < 0  # none has run
    gn, ga = sc.forward_pairs_scaled([], [])
    assert gn.shape == (0,) and ga.shape == (0,) and gn.dtype == np.float64 and sc.forward_scaled_kernel_ms < 0
    with pytest.raises(dcp.DcpError) as e:
        sc.forward_pairs_scaled([0, len(seqs), 99], [0, 0, 99])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    with pytest.raises(dcp.DcpError) as e:
        sc.forward_pairs_scaled([0, 1], [0, len(profs)])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    refused(dcp, sc, lambda: sc.forward_pairs_scaled([0, 1], [0]))
    sq, pp = np.array([0, 99], np.uint32), np.array([0, 0], np.uint32)
    null, alt = np.full(2, 1.5), np.full(2, 2.5)
    call = sc._lib.dcp_gpu_forward_pairs_scaled
    assert call(sc._c, 1, 0, sq.ctypes.data, pp.ctypes.data, 2, null.ctypes.data, alt.ctypes.data) == dcp.RC_EINVAL
    sq[1] = 1
    for args in ((None, pp.ctypes.data, null.ctypes.data, alt.ctypes.data), (sq.ctypes.data, None, null.ctypes.data, alt.ctypes.data),
                 (sq.ctypes.data, pp.ctypes.data, None, alt.ctypes.data), (sq.ctypes.data, pp.ctypes.data, null.ctypes.data, None)):
        assert call(sc._c, 1, 0, args[0], args[1], 2, args[2], args[3]) == dcp.RC_EINVAL
        assert len(sc._lib.dcp_gpu_last_error(sc._c)) > 0
    assert null.tolist() == [1.5, 1.5] and alt.tolist() == [2.5, 2.5]
    assert call(sc._c, 1, 0, None, None, 0, None, None) == 0 and sc.forward_scaled_kernel_ms < 0
    # a single pair, and a list with duplicates
    gn, ga = sc.forward_pairs_scaled([8], [9])
    want = twin(9, xtrans_of(dcp, precision, len(seqs[8]), True, False), seqs[8])
    assert within(gn, [want[0]]) and within(ga, [want[1]]) and sc.forward_scaled_kernel_ms > 0
    sq, pp = np.array([7, 8, 7, 7, 3, 8]), np.array([11, 4, 11, 11, 0, 4])
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    want = np.array([twin(p, xtrans_of(dcp, precision, len(seqs[q]), True, False), seqs[q]) for q, p in zip(sq, pp)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    assert len({int(b) for b in bits(ga)[[0, 2, 3]]}) == 1 and bits(ga)[1] == bits(ga)[5]
    # explicit transitions in the DB's precision are honoured, those of the other refused
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    sq, pp = np.array([8, 7, 4, 8, 2]), np.array([12, 9, 5, 11, 1])
    gn, ga = sc.forward_pairs_scaled(sq, pp, True, False)
    want = np.array([twin(p, xt[q], seqs[q]) for q, p in zip(sq, pp)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.forward_pairs_scaled(sq, pp))
    sc.close()

    # both strands, windows, regions
    sc = fp.loaded(dcp, precision)
    n = len(seqs)
    sc.add_reverse_strand()
    sq, pp = np.array([n + 8, n + 7, 8, n + 5]), np.array([9, 12, 9, 2])
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    want = np.array([twin(p, xtrans_of(dcp, precision, len(seqs[q % n]), True, False),
                          np_revcomp(seqs[q % n]) if q >= n else seqs[q % n]) for q, p in zip(sq, pp)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    sc.upload_seqs([seqs[8], seqs[7]])
    sc.cut_windows(64, 40)
    sq, pp = np.arange(sc.nseqs), np.arange(sc.nseqs) % len(profs)
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    want = np.array([twin(p, xtrans_of(dcp, precision, len(sc.fetch_seq(q)), True, False), sc.fetch_seq(q)) for q, p in zip(sq, pp)])
    assert sc.nseqs > 2 and within(gn, want[:, 0]) and within(ga, want[:, 1])
    sc.upload_seqs(seqs)
    sc.cut_regions([8, 8, 7], [0, 100, 30], [333, 150, 64], [0, 1, 0])
    sq, pp = np.array([0, 1, 2, 1]), np.array([10, 6, 12, 0])
    gn, ga = sc.forward_pairs_scaled(sq, pp)
    cut = [seqs[8], np_revcomp(seqs[8][100:250]), seqs[7][30:94]]
    want = np.array([twin(p, xtrans_of(dcp, precision, len(cut[q]), True, False), cut[q]) for q, p in zip(sq, pp)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_else_moves(dcp, oracle64, precision):
    profs, seqs = fp.world(dcp, precision, oracle64)[:2]
    sc = fp.loaded(dcp, precision)
    sq, pp = np.array([8, 7, 6, 8, 3]), np.array([11, 3, 0, 12, 9])

    def flat(x):
        if isinstance(x, (tuple, list)):
            return [flat(v) for v in x]
        return np.ascontiguousarray(x).tobytes()

    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    sc.forward_dense(False, False)

    def state():
        return (flat(sc.scores()), sc.hits().tobytes(), sc.cells, sc.last_scan_launches, flat(sc.forward_pairs(sq, pp)),
                flat(sc.posterior_pairs(sq, pp)), flat(sc.forward_scores()), sc.forward_dense_is_scaled)

    before = state()
    assert len(sc.hits()) > 0 and before[-1] is False
    got = sc.forward_pairs_scaled(sq, pp, False, False)  # other flags than the scan's
    assert np.isfinite(got[1]).all()
    assert state() == before
    sc.close()
