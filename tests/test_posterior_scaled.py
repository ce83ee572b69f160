"""The scaled probability-space Backward sweep and posterior rows on the host: dcp_posterior_scaled_tables (the twin of
csrc/dcp_backward_scaled.hip; the rule is csrc/dcp_backward_scaled.h).  No device: the GPU half is
tests/test_posterior_scaled_gpu.py.

The reference is dcp_posterior_tables, the log-space twin, never the code under test.

Allowances.  X is tests/test_posterior_pairs.py's X (the largest finite magnitude among the pair's alt score and the
rows' f + beta sums), A = (L (M + 2) + 2)(delta + 2^-51) with the recorded delta of the float factor rule, as in
tests/test_forward_scaled.py:
  double factors   scores 2^-32 (|x| + 1)   rows 4 x 2^-32 (X + 1)
  float factors    scores A absolute        rows 2 A + 4 x 2^-32 (X + 1)
(the exponent f + b - a carries a whole path's factor errors once in f + b and once in a; a posterior is at most about
1; core is 1 minus terms that sum to at most 1).  A sum of n posteriors gets n times the row allowance.  -inf compares
by equality; no NaN ever occurs.  Measured maxima: DESIGN section 25."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import test_forward_chain_premises as pr
import test_posterior_pairs as tp
from test_both_strands import bits
from test_forward_pairs import CODE_OFF, NEG_INF, oracle_case, within, worst
from test_forward_scaled import allowance_f32, exp_or_inf, fma, planted_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = 0.693147180559945309417232121458
SHAPES = tp.SHAPES + ((3, 5), (3, 6), (1, 9))  # and the ring's wrap (L = 5, 6), one node over several rows


def scaled(dcp, tabs, xt, seq, f32=False, band=None):
    got = dcp.posterior_scaled_tables(*tabs, xt, seq, float_factors=f32, band=band)
    assert not got[5]
    return got[:5]


def check_identities(begin, end, core, L, multi, allow):
    assert begin.shape == (L + 1,) and end[0] == 0.0 and core[0] == 0.0
    assert not np.isnan(begin).any() and not np.isnan(end).any() and not np.isnan(core).any()
    assert np.all(core >= -allow) and np.all(core <= 1.0 + allow)  # core is a probability
    n = (L + 1) * allow
    assert abs(begin.sum() - end.sum()) <= 2 * n  # begun as often as ended
    if not multi:
        assert abs(begin.sum() - 1.0) <= n  # exactly one domain in uni-hit


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_with_double_factors(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):  # float tables go in promoted
        t8, em, ei, en, xt, seq = tp.case(orc, M, L, multi)
        X = tp.restated(orc, M, L, multi)["X"]
        want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        begin, end, core, fwd, bwd = scaled(dcp, (t8, em, ei, en), xt, seq)
        w = tp.rows_within((begin, end, core), want[:3], X, (M, L, multi))
        print("scaled twin, double factors, vs posterior_tables M %d L %d multi %d f%d: scores %.3e %.3e, rows %.3e of (X + 1)" % (
            M, L, multi, 64 if orc is oracle64 else 32, worst([fwd], [want[3]]), worst([bwd], [want[4]]), w))
        assert within([fwd], [want[3]]) and within([bwd], [want[4]]) and within([bwd], [fwd])
        # alt_fwd is the scaled Forward twin's, in bits
        assert bits(np.array([fwd])) == bits(np.array([dcp.forward_scaled_tables(t8, em, ei, en, xt, seq)[1]]))
        check_identities(begin, end, core, L, multi, tp.rows_allow(X))
        for band in (4, 8):  # the band changes no bit of a pair in range
            again = scaled(dcp, (t8, em, ei, en), xt, seq, band=band)
            for g, w_ in zip(again, (begin, end, core, fwd, bwd)):
                assert np.array_equal(bits(np.atleast_1d(g)), bits(np.atleast_1d(w_))), band


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_with_float_factors(dcp, oracle32, M, L, multi):
    t8, em, ei, en, xt, seq = tp.case(oracle32, M, L, multi)
    X = tp.restated(oracle32, M, L, multi)["X"]
    want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
    begin, end, core, fwd, bwd = scaled(dcp, (t8, em, ei, en), xt, seq, f32=True)
    A = allowance_f32(L, M)
    allow = 2.0 * A + tp.rows_allow(X)
    d = max(float(np.max(np.abs(g - w))) for g, w in zip((begin, end, core), want[:3]))
    print("scaled twin, float factors, vs posterior_tables M %d L %d multi %d: scores |d| %.3e %.3e of A %.3e, rows |d| %.3e of %.3e" % (
        M, L, multi, abs(fwd - want[3]), abs(bwd - want[4]), A, d, allow))
    assert np.isfinite([fwd, bwd]).all() and abs(fwd - want[3]) <= A and abs(bwd - want[4]) <= A and abs(fwd - bwd) <= A
    assert d <= allow
    assert bits(np.array([fwd])) == bits(np.array([dcp.forward_scaled_tables(t8, em, ei, en, xt, seq, float_factors=True)[1]]))
    check_identities(begin, end, core, L, multi, allow)
    assert fwd != scaled(dcp, (t8, em, ei, en), xt, seq)[3]  # the float rule is in use


# ---- the Backward rule restated -----------------------------------------------------------------------------------
def step_of(ref, band):
    if ref == 0.0:
        return 0
    k = max((struct.unpack("<Q", struct.pack("<d", ref))[0] >> 52) & 0x7FF, 1) - 1023
    return 0 if -band <= k < band else min(k, 1022)


def score(u, s):
    if u == 0.0:
        return NEG_INF
    m, e = math.frexp(u)
    return math.log(m) + float(e + s) * LN2


def restate_backward_scaled(t8, em, ei, en, xt, seq, band):
    """dcp_backward_scaled.h's rule with double factors, in Python, for a pair that stays in range (the finiteness and
    underflow checks are left out): (alt_bwd, the records [L + 1][5] as logs, the rows after which a rescaling happened)"""
    f = exp_or_inf
    T = [[f(float(v)) for v in row] for row in np.asarray(t8, np.float64)]
    ENT, MM, IM, DM, MD, DD, MI, II = T
    RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB = (f(float(v)) for v in xt)
    em, ei, en = np.asarray(em, np.float64), np.asarray(ei, np.float64), np.asarray(en, np.float64)
    M, L = len(ENT), len(seq)
    bM, bI = [[0.0] * M for _ in range(5)], [[0.0] * M for _ in range(5)]
    bN, bJ, bC = [0.0] * 5, [0.0] * 5, [0.0] * 5
    s = step_of(max(ET, CT), band)  # row L is a row: ref = max(ET, CT), before anything reads the ring
    ETL, CTL = ET * 2.0 ** -s, CT * 2.0 ** -s
    rec, rescaled = [None] * (L + 1), []
    bB = bPN = 0.0
    for j in range(L, -1, -1):
        v, code = 0, []
        for l in range(1, 6):
            v = (v << 2) | (int(seq[j + l - 1]) if j + l - 1 < L else 0)
            code.append(CODE_OFF[l - 1] + v)
        slot = [(j + l) % 5 for l in range(1, 6)]
        fN, fI = [f(float(en[c])) for c in code], [f(float(ei[c])) for c in code]
        fM = [[f(float(x)) for x in em[c]] for c in code]
        bPN = bPJ = bPC = 0.0
        for l in range(5):
            bPN, bPJ, bPC = fma(bN[slot[l]], fN[l], bPN), fma(bJ[slot[l]], fN[l], bPJ), fma(bC[slot[l]], fN[l], bPC)
        bP, bQ = [0.0] * M, [0.0] * M
        for k in range(M):
            for l in range(5):
                bP[k] = fma(bM[slot[l]][k], fM[l][k], bP[k])
                bQ[k] = fma(bI[slot[l]][k], fI[l], bQ[k])
        bB = 0.0
        for k in range(M):
            bB += ENT[k] * bP[k]
        last = j == L
        bE = fma(EC, bPC, fma(EJ, bPJ, fma(EB, bB, ETL if last else 0.0)))
        r = j % 5
        bN[r], bJ[r], bC[r] = fma(NN, bPN, NB * bB), fma(JJ, bPJ, JB * bB), fma(CC, bPC, CTL if last else 0.0)
        bD = [0.0] * (M + 1)
        for k in range(M - 1, -1, -1):
            nx = k + 1 < M
            dn, pn = (bD[k + 1], bP[k + 1]) if nx else (0.0, 0.0)
            dd, dm, md, mm, im = (DD[k + 1], DM[k + 1], MD[k + 1], MM[k + 1], IM[k + 1]) if nx else (0.0,) * 5
            bD[k] = fma(dd, dn, fma(dm, pn, bE))
            bM[r][k] = fma(MI[k], bQ[k], fma(mm, pn, fma(md, dn, bE)))
            bI[r][k] = fma(II[k], bQ[k], im * pn)
        rec[j] = [score(x, s) for x in (bN[r], bJ[r], bC[r], bB, bE)]
        k = step_of(max(bN[r], bJ[r], bC[r], bB, bE), band)
        if k:
            c = 2.0 ** -k
            bM, bI = [[x * c for x in row] for row in bM], [[x * c for x in row] for row in bI]
            bN, bJ, bC = [x * c for x in bN], [x * c for x in bJ], [x * c for x in bC]
            bB, bPN, s = bB * c, bPN * c, s + k
            rescaled.append(j)
    k = step_of(max(bB, bPN), 0)  # the finish: the larger of the two into [1, 2), whatever the band
    alt = fma(SN, bPN * 2.0 ** -k, SB * (bB * 2.0 ** -k))
    return score(alt, s + k), rec, rescaled


@pytest.mark.parametrize("M", [2, 40])
def test_rescaling_700_nt_restated(dcp, oracle64, M):
    L = 700
    t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
    want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
    assert math.exp(want[3]) == 0.0 and math.exp(want[4]) == 0.0  # the premise: unscaled, the alt score underflows double
    begin, end, core, fwd, bwd = scaled(dcp, (t8, em, ei, en), xt, seq)
    assert within([fwd], [want[3]]) and within([bwd], [want[4]])
    X = max(abs(want[3]), abs(want[4]))  # at most test_posterior_pairs' X: a tighter allowance
    tp.rows_within((begin, end, core), want[:3], X, M)
    rows = []
    for band in (4, 64):
        alt, rec, rescaled = restate_backward_scaled(t8, em, ei, en, xt, seq, band)
        assert len(rescaled) > 3  # the rescaling is exercised
        rows.append(tuple(rescaled))
        assert bits(np.array([alt])) == bits(np.array([bwd])), band  # the twin's bits both times
        assert np.isfinite(rec[L][4]) and np.isfinite(rec[0][3])  # bE(L) and bB(0) carry weight
        got = scaled(dcp, (t8, em, ei, en), xt, seq, band=band)
        for g, w in zip(got, (begin, end, core, fwd, bwd)):
            assert np.array_equal(bits(np.atleast_1d(g)), bits(np.atleast_1d(w))), band
    assert rows[0] != rows[1]  # the two bands rescale in different rows


def test_edge_values(dcp, oracle64):
    for L in (1, 7, 10):  # epsilon = 0 and L mod 3 != 0: no path, all rows 0, the scores -inf, never NaN
        t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, L, True, eps=0.0)
        for f32 in (False, True):
            begin, end, core, fwd, bwd = scaled(dcp, (t8, em, ei, en), xt, seq, f32=f32)
            assert fwd == NEG_INF and bwd == NEG_INF
            assert not begin.any() and not end.any() and not core.any()
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 9, True, eps=0.0)
    got, want = scaled(dcp, (t8, em, ei, en), xt, seq), dcp.posterior_tables(t8, em, ei, en, xt, seq)
    assert within(got[3:], want[3:]) and got[0].sum() > 0.5
    tp.rows_within(got[:3], want[:3], abs(want[3]))
    for M, L in ((2, 7), (5, 30), (65, 60)):  # ldk > M: the bits of ldk = M
        t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
        ldk = M + 7
        t8p, emp = np.full((8, ldk), 3.0), np.full((1364, ldk), 3.0)  # padding the twin must never read as a column
        t8p[:, :M], emp[:, :M] = t8, em
        rc, out, fwd, bwd, oor = raw(dcp, M, ldk, t8p, emp, ei, en, xt, seq, L)
        assert rc == 0 and oor == 0
        want = scaled(dcp, (t8, em, ei, en), xt, seq)
        for g, w in zip(out + [np.array([fwd, bwd])], list(want[:3]) + [np.array(want[3:])]):
            assert np.array_equal(bits(g), bits(w))


def raw(dcp, M, ldk, t8, em, ei, en, xt, seq, L, f32=0, band=None, fill=1.5):
    out = [np.full(L + 1, fill) for _ in range(3)]
    fwd, bwd, oor = C.c_double(fill), C.c_double(fill), C.c_int(7)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = (M, ldk, P(t8), P(em), P(ei), P(en), P(xt), P(seq), L, f32)
    outs = (P(out[0]), P(out[1]), P(out[2]), C.byref(fwd), C.byref(bwd), C.byref(oor))
    rc = dcp.lib.dcp_posterior_scaled_tables(*args, *outs) if band is None else \
        dcp.lib.dcp_posterior_scaled_tables_band(*args, band, *outs)
    return rc, out, fwd.value, bwd.value, oor.value


def untouched(out, fwd, bwd, fill=1.5):
    return all((o == fill).all() for o in out) and fwd == fill and bwd == fill


def test_the_planted_pair_is_in_range(dcp, oracle64, oracle32):
    for orc in (oracle64, oracle32):
        t8, em, ei, en, xt, seq = planted_case(orc)
        fn, fa = dcp.forward_tables(t8, em, ei, en, xt, seq)
        assert fa - fn > 750.0  # a condition on the input
        want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        begin, end, core, fwd, bwd = scaled(dcp, (t8, em, ei, en), xt, seq)  # unflagged
        assert within([fwd], [want[3]]) and within([bwd], [want[4]])
        X = abs(want[3])  # at most test_posterior_pairs' X: a tighter allowance
        w = tp.rows_within((begin, end, core), want[:3], X)
        print("planted pair, double factors: rows %.3e of (X + 1), X %.1f; core above 0.5 on %d bases" % (w, X, int((core > 0.5).sum())))
        assert (core > 0.5).sum() > 600  # the gene is seen
        if orc is oracle32:
            got = scaled(dcp, (t8, em, ei, en), xt, seq, f32=True)
            A = allowance_f32(len(seq), 300)
            assert abs(got[3] - want[3]) <= A and abs(got[4] - want[4]) <= A
            assert max(float(np.max(np.abs(g - w_))) for g, w_ in zip(got[:3], want[:3])) <= 2.0 * A + tp.rows_allow(X)


def test_overflow_is_flagged_and_writes_nothing(dcp, oracle64):
    M, L = 2000, 12
    t8, em, ei, en, xt, seq = pr.tables(oracle64, "positive", M, L)
    assert float(np.sum(t8[5, 1:])) > 720.0  # the sum of DD: the chain multiplies up past the double range
    want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
    assert np.isfinite(want[3:]).all() and not np.isnan(want[2]).any()
    for f32 in (0, 1):
        rc, out, fwd, bwd, oor = raw(dcp, M, M, t8, em, ei, en, xt, seq, L, f32)
        assert rc == 0 and oor == 1 and untouched(out, fwd, bwd)
        assert dcp.posterior_scaled_tables(t8, em, ei, en, xt, seq, float_factors=bool(f32)) == (None,) * 5 + (True,)
    # an insert loop that multiplies up: IM = -inf, II = +96
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    t8 = t8.copy()
    t8[2], t8[7] = NEG_INF, 96.0
    assert np.isfinite(dcp.posterior_tables(t8, em, ei, en, xt, seq)[3])
    rc, out, fwd, bwd, oor = raw(dcp, 5, 5, t8, em, ei, en, xt, seq, 30)
    assert rc == 0 and oor == 1 and untouched(out, fwd, bwd)
    # the positive chain of 600 nodes stays in range
    t8, em, ei, en, xt, seq = pr.tables(oracle64, "positive", 600, 12)
    got, want = scaled(dcp, (t8, em, ei, en), xt, seq), dcp.posterior_tables(t8, em, ei, en, xt, seq)
    assert within(got[3:], want[3:])
    tp.rows_within(got[:3], want[:3], abs(want[3]))


def test_the_underflow_check_both_ways(dcp, oracle64):
    """A pair whose every path through the core costs e^-t, t = the match emissions, while N up to row j and C from row
    j on cost little: F + Bk - a is t plus the few transitions of one pass through the core at every row.  The check's
    threshold is (958 - band) ln 2: 619.7 at the default band, so t = 680 is flagged and t = 560 is not; at band 400
    (threshold 386.8) both are.  (No profile built
    through the project's constructors has emissions this low: the tables are set here, which the twin's interface
    allows.  DESIGN section 25.)"""
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    thr = lambda band: (958 - band) * LN2  # noqa: E731
    assert 560.0 + 40.0 < thr(64) < 680.0 - 40.0 and thr(400) < 560.0 - 40.0
    seen = {}
    for t in (560.0, 680.0):
        low = np.full_like(em, -t)
        want = dcp.posterior_tables(t8, low, ei, en, xt, seq)
        assert np.isfinite(want[3:]).all()
        for band in (64, 400):
            rc, out, fwd, bwd, oor = raw(dcp, 5, 5, t8, low, ei, en, xt, seq, 30, band=band)
            assert rc == 0
            seen[t, band] = oor
            if oor:
                assert untouched(out, fwd, bwd)  # a flagged pair is never returned
            else:
                assert within([fwd], [want[3]]) and within([bwd], [want[4]])
                tp.rows_within(out, want[:3], abs(want[3]))
        # the Forward sweep alone has no such check: the pair is in range for it
        assert dcp.forward_scaled_tables(t8, low, ei, en, xt, seq)[2] is False
    assert seen == {(560.0, 64): 0, (680.0, 64): 1, (560.0, 400): 1, (680.0, 400): 1}


def test_refusals_leave_the_outputs_untouched(dcp, oracle64):
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    good = dict(M=5, ldk=5, t8=t8, em=em, ei=ei, en=en, xt=xt, seq=seq, L=30)
    bad_seq = seq.copy()
    bad_seq[17] = 4
    wide = np.full((8, 4097), NEG_INF), np.full((1364, 4097), NEG_INF)
    cases = [dict(M=0), dict(M=4097, ldk=4097, t8=wide[0], em=wide[1]), dict(ldk=4), dict(L=0), dict(seq=bad_seq),
             dict(t8=None), dict(em=None), dict(ei=None), dict(en=None), dict(xt=None), dict(seq=None)]
    for change in cases:
        a = dict(good, **change)
        rc, out, fwd, bwd, oor = raw(dcp, a["M"], a["ldk"], a["t8"], a["em"], a["ei"], a["en"], a["xt"], a["seq"], a["L"])
        assert rc == dcp.RC_EINVAL and untouched(out, fwd, bwd) and oor == 7, change
    for band in (0, 501, -1):
        rc, out, fwd, bwd, oor = raw(dcp, 5, 5, t8, em, ei, en, xt, seq, 30, band=band)
        assert rc == dcp.RC_EINVAL and untouched(out, fwd, bwd) and oor == 7
    P = lambda a: a.ctypes.data  # noqa: E731
    rows = [np.full(31, 1.5) for _ in range(3)]
    d, o = C.c_double(1.5), C.c_int(7)
    full = [P(rows[0]), P(rows[1]), P(rows[2]), C.byref(d), C.byref(d), C.byref(o)]
    for missing in range(6):
        outs = [None if i == missing else v for i, v in enumerate(full)]
        assert dcp.lib.dcp_posterior_scaled_tables(5, 5, P(t8), P(em), P(ei), P(en), P(xt), P(seq), 30, 0, *outs) == dcp.RC_EINVAL
        assert all((r == 1.5).all() for r in rows) and d.value == 1.5 and o.value == 7
    with pytest.raises(dcp.DcpError):
        dcp.posterior_scaled_tables(t8, em[:, :4], ei, en, xt, seq)


def test_posterior_scaled_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_posterior_scaled.c with the host model alone (no device code) under ASan + UBSan, as a program
    of its own."""
    obj, exe = str(tmp_path / "asan_posterior_scaled.o"), str(tmp_path / "asan_posterior_scaled")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_posterior_scaled.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_posterior_scaled ok" in r.stdout
