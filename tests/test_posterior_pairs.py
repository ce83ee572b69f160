"""Backward sweep and posterior decoding of a pair list: dcp_posterior_tables (the host twin), dcp_posterior_envelopes,
dcp_gpu_posterior_pairs / Scanner.posterior_pairs.

Per pair three rows of L + 1 values: begin[j] and end[j], the posteriors that a domain begins / ends at row j, and
core[j], the posterior that base j - 1 is emitted by a core state; and the alt score by both sweeps.

CPU: a numpy restatement that holds the full matrices of both sweeps -- Backward as csrc/dcp_posterior.h states it, core
     as the direct sum of the M and I word posteriors (the host twin forms 1 - the N, J, C words) -- is what the host
     twin is held against; the identities of the rule (sums, the finite difference of the Forward score in the
     transitions into B, core a probability); epsilon 0; padding; refusals; envelopes; tests/c/asan_posterior.c under
     ASan + UBSan as a program of its own.
GPU: per precision the device against the host twin on the tables the device holds, in the world of
     tests/test_forward_pairs.py (profiles on every lane, class and chunk edge, queries of 1 .. 333 nt); agreement with
     forward_pairs in bits; few wavefronts and a small budget (hooks build); lists; other batches; explicit transitions;
     capacity; the scan untouched; the planted gene's envelope.

Allowances.  Scores: the project's 2^-32 (|x| + 1).  Posteriors: 4 x 2^-32 (X + 1) absolute, X the largest finite
magnitude among the pair's alt score and the rows' f + beta sums: the exponent f + beta - a is a sum of three values that
each carry the score allowance, and a posterior is at most about 1, so its absolute error is that of its exponent.  A
sum of n posteriors (sum begin, sum end) is held to n times that.  Measured maxima: see DESIGN section 20."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_both_strands import bits, np_revcomp, refused
from test_forward_pairs import (FLAGS, PRECISIONS, WORLD_L, WORLD_M, device_tables, loaded, oracle_case, within, world, worst,
                                xtrans_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
ALLOW = 2.0 ** -32
CODE_OFF = (0, 4, 20, 84, 340)
SHAPES = ((1, 1), (2, 1), (2, 7), (5, 30), (64, 100), (65, 60), (40, 333))  # (M, L)
X_SB, X_SN, X_NN, X_NB, X_ET, X_EC, X_CC, X_CT, X_EB, X_EJ, X_JJ, X_JB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12


def lse(terms):
    """log of the summed exponentials of the stacked terms; all -inf gives -inf"""
    c = np.stack([np.asarray(t, np.float64) for t in terms])
    m = np.max(c, axis=0)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return mm + np.log(np.sum(np.exp(c - mm), axis=0))


def word_code(seq, s, l):
    v = 0
    for b in seq[s:s + l]:
        v = (v << 2) | int(b)
    return CODE_OFF[l - 1] + v


def restate(t8, em, ei, en, xt, seq):
    """dict: alt_fwd, alt_bwd, begin, end, core (the direct sum over M and I words), occ (the five occupancies summed per
    base), X (the largest finite |alt|, |f + beta|)"""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    M, L = t8.shape[1], len(seq)
    ninf = lambda *shape: np.full(shape, NEG_INF)  # noqa: E731
    code = {(s, l): word_code(seq, s, l) for s in range(L) for l in range(1, 6) if s + l <= L}
    # ---- Forward, full matrices ----
    P, Q, Mm, Ii, Dd = (ninf(L + 1, M) for _ in range(5))
    PN, PJ, PC, B, E = (ninf(L + 1) for _ in range(5))
    PN[0], B[0] = xt[X_SN], xt[X_SB]
    P[0] = B[0] + ENT
    for j in range(1, L + 1):
        ws = [(j - l, l) for l in range(1, 6) if j - l >= 0]
        Mm[j] = lse([P[s] + em[code[s, l]] for s, l in ws])
        Ii[j] = lse([Q[s] + ei[code[s, l]] for s, l in ws])
        N = lse([PN[s] + en[code[s, l]] for s, l in ws])
        J = lse([PJ[s] + en[code[s, l]] for s, l in ws])
        Cc = lse([PC[s] + en[code[s, l]] for s, l in ws])
        for k in range(1, M):
            Dd[j, k] = lse([Mm[j, k - 1] + MD[k], Dd[j, k - 1] + DD[k]])
        E[j] = lse([Mm[j, k] for k in range(M)] + [Dd[j, k] for k in range(1, M)])
        B[j] = lse([N + xt[X_NB], E[j] + xt[X_EB], J + xt[X_JB]])
        P[j, 0] = B[j] + ENT[0]
        if M > 1:
            P[j, 1:] = lse([B[j] + ENT[1:], Mm[j, :-1] + MM[1:], Ii[j, :-1] + IM[1:], Dd[j, :-1] + DM[1:]])
        Q[j] = lse([Mm[j] + MI, Ii[j] + II])
        PN[j], PJ[j], PC[j] = N + xt[X_NN], lse([E[j] + xt[X_EJ], J + xt[X_JJ]]), lse([E[j] + xt[X_EC], Cc + xt[X_CC]])
    alt_fwd = float(lse([E[L] + xt[X_ET], Cc + xt[X_CT]]))  # C(L), after emission
    # ---- Backward, full matrices; rows past L are -inf ----
    bM, bI = ninf(L + 6, M), ninf(L + 6, M)
    bN, bJ, bC, bB, bE = (ninf(L + 6) for _ in range(5))
    bP, bQ = ninf(L + 1, M), ninf(L + 1, M)
    bPN, bPJ, bPC = ninf(L + 1), ninf(L + 1), ninf(L + 1)
    for j in range(L, -1, -1):
        ws = [l for l in range(1, 6) if j + l <= L]
        if ws:
            bP[j] = lse([em[code[j, l]] + bM[j + l] for l in ws])
            bQ[j] = lse([ei[code[j, l]] + bI[j + l] for l in ws])
            bPN[j] = lse([en[code[j, l]] + bN[j + l] for l in ws])
            bPJ[j] = lse([en[code[j, l]] + bJ[j + l] for l in ws])
            bPC[j] = lse([en[code[j, l]] + bC[j + l] for l in ws])
        bB[j] = lse(list(ENT + bP[j]))
        last = j == L
        bC[j] = lse([xt[X_CT] if last else NEG_INF, xt[X_CC] + bPC[j]])
        bJ[j] = lse([xt[X_JB] + bB[j], xt[X_JJ] + bPJ[j]])
        bN[j] = lse([xt[X_NB] + bB[j], xt[X_NN] + bPN[j]])
        bE[j] = lse([xt[X_ET] if last else NEG_INF, xt[X_EB] + bB[j], xt[X_EJ] + bPJ[j], xt[X_EC] + bPC[j]])
        bD = ninf(M + 1)
        for k in range(M - 1, -1, -1):
            nx = k + 1 < M
            dn, pn = (bD[k + 1], bP[j, k + 1]) if nx else (NEG_INF, NEG_INF)
            bD[k] = lse([bE[j], DD[k + 1] + dn if nx else NEG_INF, DM[k + 1] + pn if nx else NEG_INF])
            bM[j, k] = lse([bE[j], MD[k + 1] + dn if nx else NEG_INF, MM[k + 1] + pn if nx else NEG_INF, MI[k] + bQ[j, k]])
            bI[j, k] = lse([IM[k + 1] + pn if nx else NEG_INF, II[k] + bQ[j, k]])
    alt_bwd = float(lse([xt[X_SB] + bB[0], xt[X_SN] + bPN[0]]))
    # ---- posteriors ----
    a = alt_fwd
    begin, end, core, occ = np.zeros(L + 1), np.zeros(L + 1), np.zeros(L + 1), np.zeros(L + 1)
    sums = [a] + list(B + bB[:L + 1]) + list(E + bE[:L + 1])
    if a != NEG_INF:
        with np.errstate(invalid="ignore"):
            begin = np.exp(B + bB[:L + 1] - a)
            end = np.exp(E + bE[:L + 1] - a)
        end[0] = 0.0
        for (s, l), cd in code.items():
            wm = P[s] + em[cd] + bM[s + l]
            wi = Q[s] + ei[cd] + bI[s + l]
            wx = np.array([PN[s] + en[cd] + bN[s + l], PJ[s] + en[cd] + bJ[s + l], PC[s] + en[cd] + bC[s + l]])
            sums += list(wx)
            inside = float(np.sum(np.exp(wm - a)) + np.sum(np.exp(wi - a)))
            core[s + 1:s + l + 1] += inside
            occ[s + 1:s + l + 1] += inside + float(np.sum(np.exp(wx - a)))
    sums = np.array(sums, np.float64)
    fin = np.isfinite(sums)
    X = float(np.max(np.abs(sums[fin]))) if fin.any() else 0.0
    return dict(alt_fwd=alt_fwd, alt_bwd=alt_bwd, begin=begin, end=end, core=core, occ=occ, X=X)


def rows_allow(X):
    return 4.0 * ALLOW * (X + 1.0)


def rows_within(got, want, X, what=""):
    """(begin, end, core) within the posterior allowance; the worst |delta| / (X + 1)"""
    worst_ = 0.0
    for g, w in zip(got, want):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape and not np.isnan(g).any(), what
        d = float(np.max(np.abs(g - w))) if len(g) else 0.0
        worst_ = max(worst_, d / (X + 1.0))
        assert d <= rows_allow(X), (what, d, rows_allow(X))
    return worst_


_RESTATED, _ONE = {}, {}


def case(orc, M, L, multi, eps=0.01):
    """oracle_case of tests/test_forward_pairs.py; a one-node profile, which the oracle does not sample, from
    pfam_like_params through the oracle's constructor"""
    if M > 1:
        return oracle_case(orc, M, L, multi, eps)
    key = (orc.np, M, L, multi, eps)
    if key not in _ONE:
        from oracle_py import ENTRY_DIST_OCCUPANCY
        from test_gpu_parity import pfam_like_params
        p = orc.new(*pfam_like_params(np.random.default_rng(100 + M), M), ENTRY_DIST_OCCUPANCY, eps)
        p.setup(L, multi, False)
        _ONE[key] = p.export() + (np.random.default_rng(1000 * M + L).integers(0, 4, L, dtype=np.uint8),)
    return _ONE[key]



def restated(orc, M, L, multi, eps=0.01):
    key = (orc.np, M, L, multi, eps)
    if key not in _RESTATED:
        t8, em, ei, en, xt, seq = case(orc, M, L, multi, eps)
        _RESTATED[key] = restate(t8, em, ei, en, xt, seq)
    return _RESTATED[key]


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_against_the_restatement(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):  # float tables go in as they are: promoted to double
        t8, em, ei, en, xt, seq = case(orc, M, L, multi)
        want = restated(orc, M, L, multi)
        begin, end, core, fwd, bwd = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        null, alt = dcp.forward_tables(t8, em, ei, en, xt, seq)
        assert np.isfinite([fwd, bwd]).all()
        assert within([fwd], [alt]) and within([bwd], [alt]) and within([bwd], [fwd])
        assert within([fwd], [want["alt_fwd"]]) and within([bwd], [want["alt_bwd"]])
        assert bits(np.array([fwd])) == bits(np.array([alt]))  # one sweep, stated once
        # the restatement's own identity: every base is emitted by exactly one word of one of the five states
        assert np.max(np.abs(want["occ"][1:] - 1.0)) <= rows_allow(want["X"])
        w = rows_within((begin, end, core), (want["begin"], want["end"], want["core"]), want["X"], (M, L, multi))
        print("host twin vs restatement M %d L %d multi %d f%d: scores %.3e %.3e, rows %.3e of (X + 1), X %.1f" % (
            M, L, multi, 64 if orc is oracle64 else 32, worst([fwd], [want["alt_fwd"]]), worst([bwd], [want["alt_bwd"]]), w,
            want["X"]))
        assert begin.shape == (L + 1,) and end[0] == 0.0 and core[0] == 0.0
        # core is a probability
        assert np.all(core >= -rows_allow(want["X"])) and np.all(core <= 1.0 + rows_allow(want["X"]))
        # the expected number of domains: begun as often as ended; exactly one in uni-hit
        n = (L + 1) * rows_allow(want["X"])
        assert abs(begin.sum() - end.sum()) <= 2 * n
        if not multi:
            assert abs(begin.sum() - 1.0) <= n


@pytest.mark.parametrize("M,L", SHAPES)
def test_domains_begun_are_the_forward_scores_slope(dcp, oracle64, M, L):
    """multi-hit: every domain passes one transition into B, so sum begin is the derivative of the Forward alt score
    along (SB, NB, EB, JB) -- central quotients of forward_tables at h = 2^-10 and 2^-11, Richardson-combined.  The
    truncation is O(h^4), the rounding about 1e-14 |alt| / h: both orders below the allowance of 1e-6."""
    t8, em, ei, en, xt, seq = case(oracle64, M, L, True)
    begin = dcp.posterior_tables(t8, em, ei, en, xt, seq)[0]
    into_b = [i for i in (X_SB, X_NB, X_EB, X_JB) if np.isfinite(xt[i])]

    def quotient(h):
        up, down = np.array(xt, np.float64), np.array(xt, np.float64)
        up[into_b] += h
        down[into_b] -= h
        return (dcp.forward_tables(t8, em, ei, en, up, seq)[1] - dcp.forward_tables(t8, em, ei, en, down, seq)[1]) / (2 * h)

    slope = (4.0 * quotient(2.0 ** -11) - quotient(2.0 ** -10)) / 3.0
    print("sum begin %.12f, slope %.12f, gap %.3e (M %d L %d)" % (begin.sum(), slope, abs(begin.sum() - slope), M, L))
    assert abs(begin.sum() - slope) <= 1e-6


def test_epsilon_zero_is_all_zero_not_nan(dcp, oracle64):
    for L in (1, 7, 10):  # L mod 3 != 0: no path emits the sequence in codons alone
        t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, L, True, eps=0.0)
        begin, end, core, fwd, bwd = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        assert fwd == NEG_INF and bwd == NEG_INF
        assert not begin.any() and not end.any() and not core.any()
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 9, True, eps=0.0)
    begin, end, core, fwd, bwd = dcp.posterior_tables(t8, em, ei, en, xt, seq)
    assert np.isfinite([fwd, bwd]).all() and begin.sum() > 0.5 and not np.isnan(core).any()


def raw_posterior(dcp, M, ldk, t8, em, ei, en, xt, seq, L, fill=1.5):
    out = [np.full(L + 1, fill) for _ in range(3)]
    fwd, bwd = C.c_double(fill), C.c_double(fill)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = dcp.lib.dcp_posterior_tables(M, ldk, P(t8), P(em), P(ei), P(en), P(xt), P(seq), L, P(out[0]), P(out[1]), P(out[2]),
                                      C.byref(fwd), C.byref(bwd))
    return rc, out, fwd.value, bwd.value


def test_padding_columns_change_no_bit(dcp, oracle64):
    for M, L in ((2, 7), (5, 30), (65, 60)):
        t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
        ldk = M + 7
        t8p, emp = np.full((8, ldk), NEG_INF), np.full((1364, ldk), NEG_INF)
        t8p[:, :M], emp[:, :M] = t8, em
        want = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        rc, out, fwd, bwd = raw_posterior(dcp, M, ldk, t8p, emp, ei, en, xt, seq, L)
        assert rc == 0
        for g, w in zip(out + [np.array([fwd, bwd])], list(want[:3]) + [np.array(want[3:])]):
            assert np.array_equal(bits(g), bits(w))


def test_host_twin_refusals_write_nothing(dcp, oracle64):
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    good = dict(M=5, ldk=5, t8=t8, em=em, ei=ei, en=en, xt=xt, seq=seq, L=30)
    bad_seq = seq.copy()
    bad_seq[17] = 4
    wide = np.full((8, 4097), NEG_INF), np.full((1364, 4097), NEG_INF)
    cases = [dict(M=0), dict(M=4097, ldk=4097, t8=wide[0], em=wide[1]), dict(ldk=4), dict(L=0), dict(seq=bad_seq),
             dict(t8=None), dict(em=None), dict(ei=None), dict(en=None), dict(xt=None), dict(seq=None)]
    for change in cases:
        a = dict(good, **change)
        rc, out, fwd, bwd = raw_posterior(dcp, a["M"], a["ldk"], a["t8"], a["em"], a["ei"], a["en"], a["xt"], a["seq"], a["L"])
        assert rc == dcp.RC_EINVAL and (fwd, bwd) == (1.5, 1.5) and all((o == 1.5).all() for o in out), change
    P = lambda a: a.ctypes.data  # noqa: E731
    for missing in range(5):
        outs = [np.full(31, 1.5) for _ in range(3)] + [np.full(1, 1.5), np.full(1, 1.5)]
        ptrs = [None if i == missing else P(o) for i, o in enumerate(outs)]
        ptrs[3:] = [C.cast(p, C.POINTER(C.c_double)) for p in ptrs[3:]]
        assert dcp.lib.dcp_posterior_tables(5, 5, P(t8), P(em), P(ei), P(en), P(xt), P(seq), 30, *ptrs) == dcp.RC_EINVAL
        assert all((o == 1.5).all() for o in outs)
    with pytest.raises(dcp.DcpError):
        dcp.posterior_tables(t8, em[:, :4], ei, en, xt, seq)


def test_envelopes_on_hand_made_rows(dcp):
    env = dcp.posterior_envelopes
    row = lambda *v: np.array((0.0,) + v)  # noqa: E731  (core[0] belongs to no base)
    assert env(row()) == []  # no base at all
    assert env(row(0.9, 0.8, 0.5)) == [(0, 3)]  # all above; the threshold itself counts
    assert env(row(0.1, 0.2, 0.49)) == []
    assert env(row(0.9, 0.9, 0.1, 0.1)) == [(0, 2)] and env(row(0.1, 0.1, 0.9, 0.9)) == [(2, 4)]  # a run at either end
    r = row(0.9, 0.1, 0.8, 0.8, 0.0, 0.7, 0.7, 0.7, 0.2, 0.6)
    assert env(r) == [(0, 1), (2, 4), (5, 8), (9, 10)]
    assert env(r, min_len=2) == [(2, 4), (5, 8)] and env(r, min_len=3) == [(5, 8)] and env(r, min_len=4) == []
    assert env(r, threshold=0.75) == [(0, 1), (2, 4)] and env(r, threshold=0.0) == [(0, 10)]
    assert env(np.array([1.0, 0.0, 0.0])) == []  # core[0] is no base's
    # cap smaller than the count: the true count comes back, the first cap intervals are written
    b, e, n = np.full(4, 77, np.uint32), np.full(4, 77, np.uint32), C.c_uint(0)
    assert dcp.lib.dcp_posterior_envelopes(r.ctypes.data, 10, 0.5, 1, b.ctypes.data, e.ctypes.data, 2, C.byref(n)) == 0
    assert n.value == 4 and b.tolist() == [0, 2, 77, 77] and e.tolist() == [1, 4, 77, 77]
    assert dcp.lib.dcp_posterior_envelopes(r.ctypes.data, 10, 0.5, 1, None, None, 0, C.byref(n)) == 0 and n.value == 4
    assert dcp.lib.dcp_posterior_envelopes(None, 0, 0.5, 1, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # refusals
    n = C.c_uint(9)
    assert dcp.lib.dcp_posterior_envelopes(r.ctypes.data, 10, 0.5, 1, None, e.ctypes.data, 2, C.byref(n)) == dcp.RC_EINVAL
    assert dcp.lib.dcp_posterior_envelopes(None, 10, 0.5, 1, b.ctypes.data, e.ctypes.data, 2, C.byref(n)) == dcp.RC_EINVAL
    assert dcp.lib.dcp_posterior_envelopes(r.ctypes.data, 10, float("nan"), 1, b.ctypes.data, e.ctypes.data, 2,
                                           C.byref(n)) == dcp.RC_EINVAL
    assert dcp.lib.dcp_posterior_envelopes(r.ctypes.data, 10, 0.5, 1, b.ctypes.data, e.ctypes.data, 2, None) == dcp.RC_EINVAL
    assert n.value == 9
    with pytest.raises(dcp.DcpError):
        env(np.zeros(0))


def test_posterior_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_posterior.c with the host model alone (no device code) under ASan + UBSan, as a program of its
    own."""
    obj, exe = str(tmp_path / "asan_posterior.o"), str(tmp_path / "asan_posterior")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_posterior.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_posterior ok" in r.stdout


# ---- GPU: the device against the host twin -----------------------------------------------------------------------
_REF = {}


def twin_rows(dcp, tabs, xt, seq):
    """the host twin's (begin, end, core, alt_fwd, alt_bwd) and X, the largest finite magnitude among the alt score
    and the rows' f + beta sums, read back from the rows themselves: f + beta = a + log(posterior)"""
    begin, end, core, fwd, bwd = dcp.posterior_tables(*tabs, xt, seq)
    X = abs(fwd) if np.isfinite(fwd) else 0.0
    if np.isfinite(fwd):
        for row in (begin, end):
            pos = row[row > 0.0]
            if len(pos):
                X = max(X, float(np.max(np.abs(fwd + np.log(pos)))))
    return begin, end, core, fwd, bwd, X


def reference(dcp, precision, orc64):
    """per flags and (q, p): the host twin on the tables the device holds; computed once"""
    if precision not in _REF:
        profs, seqs, tabs = world(dcp, precision, orc64)[:3]
        ref = {}
        for multi, h3 in FLAGS:
            for q, s in enumerate(seqs):
                xt = xtrans_of(dcp, precision, len(s), multi, h3)
                for p in range(len(profs)):
                    ref[multi, h3, q, p] = twin_rows(dcp, tabs[p], xt, s)
        _REF[precision] = ref
    return _REF[precision]


def unpack(res):
    """[(begin, end, core)] per pair, alt_fwd, alt_bwd, and the offsets checked"""
    row_off, begin, end, core, fwd, bwd = res
    assert row_off.dtype == np.uint64 and row_off[0] == 0 and len(row_off) == len(fwd) + 1 and row_off[-1] == len(begin)
    assert begin.dtype == end.dtype == core.dtype == np.float64 and len(begin) == len(end) == len(core)
    o = row_off.astype(np.int64)
    return [(begin[o[i]:o[i + 1]], end[o[i]:o[i + 1]], core[o[i]:o[i + 1]]) for i in range(len(fwd))], fwd, bwd


def same_bits(x, y):
    return all(np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b))) for a, b in zip(x, y))


def check_against(rows, fwd, bwd, wants, what):
    """every pair within the allowances of its reference (begin, end, core, alt_fwd, alt_bwd, X); the worst ratios"""
    ws, wr = 0.0, 0.0
    for i, want in enumerate(wants):
        assert within([fwd[i]], [want[3]]) and within([bwd[i]], [want[4]]), (what, i, fwd[i], bwd[i], want[3], want[4])
        assert within([bwd[i]], [fwd[i]])
        assert len(rows[i][0]) == len(want[0])
        ws = max(ws, worst([fwd[i]], [want[3]]), worst([bwd[i]], [want[4]]))
        wr = max(wr, rows_within(rows[i], want[:3], want[5], (what, i)))
    return ws, wr


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pair_against_the_host_twin(dcp, oracle64, precision, multi, h3):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    ref = reference(dcp, precision, oracle64)
    every = [(q, p) for q in range(len(seqs)) for p in range(len(profs))]
    order = np.random.default_rng(12).permutation(len(every))
    sq, pr = np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])
    sc = loaded(dcp, precision)
    res = sc.posterior_pairs(sq, pr, multi, h3)
    assert sc.posterior_kernel_ms > 0
    null, alt = sc.forward_pairs(sq, pr, multi, h3)
    sc.close()
    rows, fwd, bwd = unpack(res)
    assert [len(r[0]) for r in rows] == [len(seqs[q]) + 1 for q in sq]
    assert np.array_equal(bits(fwd), bits(alt))  # one sweep: the bits of forward_pairs
    ws, wr = check_against(rows, fwd, bwd, [ref[multi, h3, q, p] for q, p in zip(sq, pr)], (precision, multi, h3))
    print("device vs host twin f%d multi %d h3 %d: scores %.3e, rows %.3e of (X + 1)" % (precision, multi, h3, ws, wr))
    assert np.isfinite(fwd).sum() > len(every) // 2
    for (b, e, c), a in zip(rows, fwd):
        assert b.shape == e.shape == c.shape and e[0] == 0.0 and c[0] == 0.0
        if a == NEG_INF:
            assert not b.any() and not e.any() and not c.any()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_few_wavefronts_and_a_small_budget_change_no_bit(dcp, oracle64, precision):
    """the stride loop's second trip, a wide pair behind a narrower one in the same work area; rounds of a few pairs, a
    pair larger than the budget in a round of its own"""
    profs, seqs = world(dcp, precision, oracle64)[:2]
    ref = reference(dcp, precision, oracle64)
    ix = {M: i for i, M in enumerate(WORLD_M)}
    q = WORLD_L.index(100)
    pairs = [(q, ix[1100]), (q, ix[257]), (q, ix[1100]), (q, ix[2]), (q, ix[513])]
    pairs += [(8, ix[512]), (7, ix[64]), (8, ix[129]), (5, ix[1100]), (8, len(WORLD_M)), (6, ix[256]), (0, ix[63]), (3, ix[128])]
    sq, pr = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    sc = loaded(dcp, precision, dcp.load_testhooks())
    base = sc.posterior_pairs(sq, pr)
    rows, fwd, bwd = unpack(base)
    check_against(rows, fwd, bwd, [ref[True, False, a, b] for a, b in pairs], precision)
    for cap in (3, 1, 0):
        sc.test_set_forward_waves(cap)
        assert same_bits(sc.posterior_pairs(sq, pr), base), cap
    # 80 bytes of records a row: rounds of at most 250 and of at most 20 rows (every pair of 100 or 333 nt alone)
    for budget in (250 * 80, 20 * 80, 1, 0):
        sc.test_set_posterior_budget(budget)
        assert same_bits(sc.posterior_pairs(sq, pr), base), budget
    sc.test_set_posterior_budget(250 * 80)
    sc.test_set_forward_waves(1)
    assert same_bits(sc.posterior_pairs(sq, pr), base)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lists_come_back_in_list_order(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    ref = reference(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    assert sc.posterior_kernel_ms < 0  # none has run
    row_off, begin, end, core, fwd, bwd = sc.posterior_pairs([], [])
    assert row_off.tolist() == [0] and begin.shape == end.shape == core.shape == fwd.shape == bwd.shape == (0,)
    assert sc.posterior_kernel_ms < 0 and sc.forward_kernel_ms < 0
    rows, fwd, bwd = unpack(sc.posterior_pairs([8], [9]))
    check_against(rows, fwd, bwd, [ref[True, False, 8, 9]], precision)
    assert sc.posterior_kernel_ms > 0 and sc.forward_kernel_ms < 0  # forward_pairs' clock is its own
    sq, pr = np.array([7, 8, 7, 7, 3, 8]), np.array([11, 4, 11, 11, 0, 4])
    res = sc.posterior_pairs(sq, pr)
    assert res[0].tolist() == np.concatenate([[0], np.cumsum([len(seqs[q]) + 1 for q in sq])]).tolist()
    rows, fwd, bwd = unpack(res)
    check_against(rows, fwd, bwd, [ref[True, False, a, b] for a, b in zip(sq, pr)], precision)
    assert same_bits(rows[0], rows[2]) and same_bits(rows[0], rows[3]) and same_bits(rows[1], rows[5])  # listed twice: scored twice
    assert bits(bwd)[0] == bits(bwd)[2] == bits(bwd)[3]
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_batches(dcp, oracle64, precision):
    profs, seqs, tabs = world(dcp, precision, oracle64)[:3]
    ref = reference(dcp, precision, oracle64)
    from oracle_py import ENTRY_DIST_OCCUPANCY
    eps0 = dcp.ProteinProfile.sample(77, 70, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    mine = [profs[3], eps0, profs[8], profs[12]]
    sc = dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs(seqs)
    mytabs = device_tables(dcp, sc, mine, precision, 0.0)[1]
    sq, pr = np.arange(len(seqs)).repeat(4), np.tile(np.arange(4), len(seqs))
    rows, fwd, bwd = unpack(sc.posterior_pairs(sq, pr))
    wants = []
    for q, s in enumerate(seqs):
        wants += [ref[True, False, q, 3], twin_rows(dcp, mytabs, xtrans_of(dcp, precision, len(s), True, False), s),
                  ref[True, False, q, 8], ref[True, False, q, 12]]
        if len(s) % 3:  # epsilon 0: no path, all rows 0
            assert fwd[4 * q + 1] == NEG_INF and bwd[4 * q + 1] == NEG_INF and not any(r.any() for r in rows[4 * q + 1])
    check_against(rows, fwd, bwd, wants, precision)
    sc.close()

    # both strands: resident n + q is the reverse complement of q
    sc = loaded(dcp, precision)
    n = len(seqs)
    sc.add_reverse_strand()
    sq, pr = np.array([n + 8, n + 7, 8, n + 5]), np.array([9, 12, 9, 2])
    rows, fwd, bwd = unpack(sc.posterior_pairs(sq, pr))
    wants = [twin_rows(dcp, tabs[p], xtrans_of(dcp, precision, len(seqs[q % n]), True, False),
                       np_revcomp(seqs[q % n]) if q >= n else seqs[q % n]) for q, p in zip(sq, pr)]
    check_against(rows, fwd, bwd, wants, precision)
    sc.close()

    # regions cut out of the batch
    sc = loaded(dcp, precision)
    sc.cut_regions([8, 8, 7], [0, 100, 30], [333, 150, 64], [0, 1, 0])
    sq, pr = np.array([0, 1, 2, 1]), np.array([10, 6, 12, 0])
    cut = [seqs[8], np_revcomp(seqs[8][100:250]), seqs[7][30:94]]
    rows, fwd, bwd = unpack(sc.posterior_pairs(sq, pr))
    wants = [twin_rows(dcp, tabs[p], xtrans_of(dcp, precision, len(cut[q]), True, False), cut[q]) for q, p in zip(sq, pr)]
    check_against(rows, fwd, bwd, wants, precision)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_transitions_in_the_dbs_precision(dcp, oracle64, precision):
    profs, seqs, tabs = world(dcp, precision, oracle64)[:3]
    ref = reference(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    sq, pr = np.array([8, 7, 4, 8, 2]), np.array([12, 9, 5, 11, 1])
    rows, fwd, bwd = unpack(sc.posterior_pairs(sq, pr, True, False))  # the flags are ignored
    check_against(rows, fwd, bwd, [twin_rows(dcp, tabs[p], xt[q], seqs[q]) for q, p in zip(sq, pr)], precision)
    assert not within(fwd, [ref[True, False, q, p][3] for q, p in zip(sq, pr)])
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.posterior_pairs(sq, pr))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_and_capacity_leave_the_outputs(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.posterior_pairs([0], [0]))  # no DB
    sc.upload_db(profs)
    refused(dcp, sc, lambda: sc.posterior_pairs([0], [0]))  # no batch
    sc.upload_seqs(seqs)
    with pytest.raises(dcp.DcpError) as e:
        sc.posterior_pairs([0, len(seqs), 99], [0, 0, 99])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    with pytest.raises(dcp.DcpError) as e:
        sc.posterior_pairs([0, 1], [0, len(profs)])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    refused(dcp, sc, lambda: sc.posterior_pairs([0, 1], [0]))
    sq, pr = np.array([8, 5], np.uint32), np.array([0, 3], np.uint32)
    need = len(seqs[8]) + len(seqs[5]) + 2
    off = np.full(3, 7, np.uint64)
    rows = [np.full(need, 1.5) for _ in range(3)]
    fwd, bwd = np.full(2, 2.5), np.full(2, 2.5)
    call = sc._lib.dcp_gpu_posterior_pairs
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def run(sq_=sq, pr_=pr, off_=off, rows_=rows, cap=need, fwd_=fwd, bwd_=bwd, n=2):
        return call(sc._c, 1, 0, P(sq_), P(pr_), n, P(off_), P(rows_[0]), P(rows_[1]), P(rows_[2]), cap, P(fwd_), P(bwd_))

    def untouched():
        return off.tolist() == [7, 7, 7] and all((r == 1.5).all() for r in rows) and (fwd == 2.5).all() and (bwd == 2.5).all()

    # capacity one short: refused, the message names the need
    assert run(cap=need - 1) == dcp.RC_EINVAL and untouched()
    assert str(need) in sc._lib.dcp_gpu_last_error(sc._c).decode()
    for change in (dict(sq_=None), dict(pr_=None), dict(off_=None), dict(rows_=[None, rows[1], rows[2]]),
                   dict(rows_=[rows[0], None, rows[2]]), dict(rows_=[rows[0], rows[1], None]), dict(fwd_=None), dict(bwd_=None),
                   dict(sq_=np.array([8, 99], np.uint32))):
        assert run(**change) == dcp.RC_EINVAL and untouched(), change
        assert len(sc._lib.dcp_gpu_last_error(sc._c)) > 0
    assert sc.posterior_kernel_ms < 0
    assert run() == 0
    assert off.tolist() == [0, len(seqs[8]) + 1, need] and np.isfinite(fwd).all() and not (rows[0] == 1.5).any()
    assert sc.posterior_kernel_ms > 0
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_scan_and_forward_pairs_are_untouched(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    ref = reference(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    nl, al = sc.scores()
    hits, cells, launches = sc.hits().copy(), sc.cells, sc.last_scan_launches
    assert len(hits) > 0
    sq, pr = np.array([8, 7, 6, 8]), np.array([11, 3, 0, 12])
    f0 = sc.forward_pairs(sq, pr, False, False)
    ms = sc.forward_kernel_ms
    rows, fwd, bwd = unpack(sc.posterior_pairs(sq, pr, False, False))  # other flags than the scan's
    check_against(rows, fwd, bwd, [ref[False, False, a, b] for a, b in zip(sq, pr)], precision)
    assert abs(sc.forward_kernel_ms - ms) <= 1e-3 * ms  # forward_pairs' events are its own (read twice: float rounding)
    f1 = sc.forward_pairs(sq, pr, False, False)
    assert same_bits(f0, f1) and np.array_equal(bits(fwd), bits(f0[1]))
    n2, a2 = sc.scores()
    assert np.array_equal(bits(n2), bits(nl)) and np.array_equal(bits(a2), bits(al))
    assert sc.hits().tobytes() == hits.tobytes() and sc.cells == cells and sc.last_scan_launches == launches
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_planted_genes_envelope(dcp, oracle32, oracle64, precision):
    """the 333-nt query of tests/test_scan_pairs.py carries the 64-node profile's gene in bases [70, 262): the envelope
    at threshold 0.5 overlaps it.  Found on the device: one envelope, [70, 262) itself on the float DB and on the double
    DB -- stated, not gated."""
    from test_scan_pairs import pair_world
    profs, seqs = pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)[:2]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    rows, fwd, bwd = unpack(sc.posterior_pairs([5], [1]))
    sc.close()
    begin, end, core = rows[0]
    env = dcp.posterior_envelopes(core, 0.5)
    overlap = sum(max(0, min(e, 262) - max(b, 70)) for b, e in env)
    print("planted gene [70, 262) f%d: envelopes %s, overlap %d bases, expected domains %.4f" % (precision, env, overlap,
                                                                                                 begin.sum()))
    assert overlap > 0
    assert within([bwd[0]], [fwd[0]])
