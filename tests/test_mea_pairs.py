"""The posterior-decoded (maximum expected accuracy) alignment of a pair list: dcp_mea_tables and dcp_mea_path_gain (the
host twins), dcp_gpu_mea_pairs / Scanner.mea_pairs.

The gain of a path is the sum of seqlen x word posterior over its emitting steps; the decoded path is an S .. T path over
finite transitions and emissions that emits the whole sequence and has the largest gain (csrc/dcp_mea.h).

CPU: an enumerator of all admissible paths on tiny shapes (validated on its own: the summed weights give the Forward
     score) gives the word posteriors and the best gain by brute force; a numpy restatement of the max-plus sweep on the
     full matrices of the two sweeps (those of tests/test_posterior_pairs.py's restate, recomputed here and held to its
     scores in bits); the Viterbi path is no better than the decoded one; epsilon 0; padding; refusals;
     tests/c/asan_mea.c under ASan + UBSan as a program of its own.
GPU: per precision the device against the host twin on the tables the device holds, in the world of
     tests/test_forward_pairs.py: the device's path is judged on the host's numbers by mea_path_gain.

Tolerance (derived, not measured).  allow(X) = 4 x 2^-32 (X + 1) is the posterior allowance of
tests/test_posterior_pairs.py, X the largest of |a| and |a + log w| over the steps with w > 0.  A word of l <= 5 bases
adds l w to the gain, so a path of n emitting steps has its gain known to 5 n allow(X) on either side; the device's path,
optimal on the device's numbers, may therefore fall short of the host's optimum by 5 (n_dev + n_host) allow(X) when both
are evaluated on the host's numbers -- and never exceeds it: max is exact.  Measured ratios: DESIGN section 22."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, np_revcomp, refused
from test_forward_pairs import FLAGS, PRECISIONS, WORLD_L, WORLD_M, device_tables, loaded, oracle_case, within, world, xtrans_of
from test_posterior_pairs import SHAPES, case, restate, rows_allow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
CODE_OFF = (0, 4, 20, 84, 340)
X_SB, X_SN, X_NN, X_NB, X_ET, X_EC, X_CC, X_CT, X_EB, X_EJ, X_JJ, X_JB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
EXT = 3 << 14
S_, N_, B_, E_, J_, C_, T_ = (EXT | i for i in (1, 2, 3, 4, 5, 6, 7))
ENUM_SHAPES = ((1, 1), (1, 2), (2, 2), (2, 3), (3, 4))


def allow(X):
    return rows_allow(X)


def tol(n, X):
    """what the gain of a path of n emitting steps is known to"""
    return 5.0 * n * allow(X)


def emitting(steps):
    return int(np.count_nonzero(steps["seqlen"]))


def path_x(a, post):
    """X read back from a path's posteriors: f + e + beta = a + log w"""
    post = np.asarray(post, np.float64)
    pos = post[post > 0.0]
    return max(abs(a), float(np.max(np.abs(a + np.log(pos)))) if len(pos) else 0.0)


def word_code(seq, s, l):
    v = 0
    for b in seq[s:s + l]:
        v = (v << 2) | int(b)
    return CODE_OFF[l - 1] + v


def as_steps(dcp, pairs):
    out = np.zeros(len(pairs), dcp.STEP_DTYPE)
    out["state_id"], out["seqlen"] = [p[0] for p in pairs], [p[1] for p in pairs]
    return out


def well_formed(steps, L):
    assert steps["state_id"][0] == S_ and steps["state_id"][-1] == T_ and int(steps["seqlen"].sum()) == L
    assert not steps["reserved"].any()


# ---- the enumerator: every admissible path of a tiny pair ---------------------------------------------------------------
def enumerate_paths(t8, em, ei, en, xt, seq):
    """[(steps, log weight)] of all S .. T paths over finite transitions and emissions that emit the whole sequence;
    steps are (state_id, seqlen) in trace_paths' conventions"""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    M, L = t8.shape[1], len(seq)
    out = []
    special = {"PN": (N_, "N"), "PJ": (J_, "J"), "PC": (C_, "C")}

    def go(state, k, pos, steps, w):
        if w == NEG_INF:
            return
        if state in special:
            sid, after = special[state]
            for l in range(1, 6):
                if pos + l <= L:
                    go(after, 0, pos + l, steps + [(sid, l)], w + en[word_code(seq, pos, l)])
        elif state == "N":
            go("B", 0, pos, steps, w + xt[X_NB])
            go("PN", 0, pos, steps, w + xt[X_NN])
        elif state == "J":
            go("B", 0, pos, steps, w + xt[X_JB])
            go("PJ", 0, pos, steps, w + xt[X_JJ])
        elif state == "C":
            if pos == L:
                go("T", 0, pos, steps, w + xt[X_CT])
            go("PC", 0, pos, steps, w + xt[X_CC])
        elif state == "B":
            for kk in range(M):
                go("P", kk, pos, steps + [(B_, 0)], w + ENT[kk])
        elif state == "P":
            for l in range(1, 6):
                if pos + l <= L:
                    go("M", k, pos + l, steps + [(k + 1, l)], w + em[word_code(seq, pos, l), k])
        elif state == "Q":
            for l in range(1, 6):
                if pos + l <= L:
                    go("I", k, pos + l, steps + [((1 << 14) | (k + 1), l)], w + ei[word_code(seq, pos, l)])
        elif state == "M":
            go("E", 0, pos, steps, w)
            if k + 1 < M:
                go("D", k + 1, pos, steps, w + MD[k + 1])
                go("P", k + 1, pos, steps, w + MM[k + 1])
            go("Q", k, pos, steps, w + MI[k])
        elif state == "I":
            if k + 1 < M:
                go("P", k + 1, pos, steps, w + IM[k + 1])
            go("Q", k, pos, steps, w + II[k])
        elif state == "D":
            steps = steps + [((2 << 14) | (k + 1), 0)]
            go("E", 0, pos, steps, w)
            if k + 1 < M:
                go("D", k + 1, pos, steps, w + DD[k + 1])
                go("P", k + 1, pos, steps, w + DM[k + 1])
        elif state == "E":
            steps = steps + [(E_, 0)]
            if pos == L:
                go("T", 0, pos, steps, w + xt[X_ET])
            go("B", 0, pos, steps, w + xt[X_EB])
            go("PJ", 0, pos, steps, w + xt[X_EJ])
            go("PC", 0, pos, steps, w + xt[X_EC])
        else:  # T
            out.append((steps + [(T_, 0)], w))

    go("B", 0, 0, [(S_, 0)], 0.0 + xt[X_SB])
    go("PN", 0, 0, [(S_, 0)], 0.0 + xt[X_SN])
    return out


def words_of(steps):
    """[(state_id, first base, seqlen)] of the emitting steps"""
    out, pos = [], 0
    for sid, l in steps:
        if l:
            out.append((sid, pos, l))
        pos += l
    return out


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", ENUM_SHAPES)
def test_enumeration_of_all_paths(dcp, oracle64, M, L, multi):
    t8, em, ei, en, xt, seq = case(oracle64, M, L, multi)
    paths = enumerate_paths(t8, em, ei, en, xt, seq)
    assert len(paths) > 0 and len({tuple(p) for p, _ in paths}) == len(paths)
    ws = np.array([w for _, w in paths])
    a = float(np.max(ws) + np.log(np.sum(np.exp(ws - np.max(ws)))))
    steps, post, gain, fwd = dcp.mea_tables(t8, em, ei, en, xt, seq)
    # the enumerator on its own: all paths together weigh the Forward score
    assert within([a], [fwd]) and within([a], [dcp.forward_tables(t8, em, ei, en, xt, seq)[1]])
    # word posteriors by summing the weights of the paths that hold the word
    wpost = {}
    for p, w in paths:
        for key in words_of(p):
            wpost[key] = wpost.get(key, 0.0) + math.exp(w - a)
    X = max([abs(a)] + [abs(a + math.log(v)) for v in wpost.values() if v > 0.0])
    occ = np.zeros(L)
    for (sid, s, l), v in wpost.items():
        occ[s:s + l] += v
    assert np.max(np.abs(occ - 1.0)) <= len(wpost) * allow(X)  # every base is emitted by exactly one word
    seen, worst_w = set(), 0.0
    for p, w in paths:  # one path per word is enough to read every word's posterior from mea_path_gain
        keys = words_of(p)
        if all(k in seen for k in keys):
            continue
        seen.update(keys)
        g, ps = dcp.mea_path_gain(t8, em, ei, en, xt, seq, as_steps(dcp, p))
        ps_e = ps[np.array([l for _, l in p]) > 0]
        assert (ps[np.array([l for _, l in p]) == 0] == -1.0).all()
        for key, v in zip(keys, ps_e):
            worst_w = max(worst_w, abs(v - wpost[key]) / (X + 1.0))
            assert abs(v - wpost[key]) <= allow(X), (key, v, wpost[key])
        assert abs(g - sum(k[2] * wpost[k] for k in keys)) <= tol(len(keys), X)
    assert seen == set(wpost)
    # the best gain by brute force
    gains = [sum(k[2] * wpost[k] for k in words_of(p)) for p, _ in paths]
    best = int(np.argmax(gains))
    n_best, n_host = len(words_of(paths[best][0])), emitting(steps)
    print("enumeration M %d L %d multi %d: %d paths, %d words, best gain %.12f, host %.12f, gap %.3e of %.3e, words %.3e of "
          "(X + 1)" % (M, L, multi, len(paths), len(wpost), gains[best], gain, abs(gains[best] - gain),
                       tol(n_best + n_host, X), worst_w))
    assert abs(gains[best] - gain) <= tol(n_best + n_host, X)
    well_formed(steps, L)
    assert tuple(zip(steps["state_id"].tolist(), steps["seqlen"].tolist())) in {tuple(p) for p, _ in paths}
    assert 0.0 <= gain <= L + L * allow(X)


# ---- the restatement: the max-plus sweep on the full matrices of both sweeps ------------------------------------------
def lse(terms):
    c = np.stack([np.asarray(t, np.float64) for t in terms])
    m = np.max(c, axis=0)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return mm + np.log(np.sum(np.exp(c - mm), axis=0))


def matrices(t8, em, ei, en, xt, seq):
    """the two sweeps of tests/test_posterior_pairs.py's restate, operation for operation, with their matrices handed out:
    P, Q, PN, PJ, PC, bM, bI, bN, bJ, bC (the Backward ones with rows L + 1 .. L + 5 of -inf), alt_fwd, alt_bwd"""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    M, L = t8.shape[1], len(seq)
    ninf = lambda *shape: np.full(shape, NEG_INF)  # noqa: E731
    code = {(s, l): word_code(seq, s, l) for s in range(L) for l in range(1, 6) if s + l <= L}
    P, Q, Mm, Ii, Dd = (ninf(L + 1, M) for _ in range(5))
    PN, PJ, PC, B, E = (ninf(L + 1) for _ in range(5))
    PN[0], B[0] = xt[X_SN], xt[X_SB]
    P[0] = B[0] + ENT
    Cc = NEG_INF
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
    alt_fwd = float(lse([E[L] + xt[X_ET], Cc + xt[X_CT]]))
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
    return dict(P=P, Q=Q, PN=PN, PJ=PJ, PC=PC, bM=bM, bI=bI, bN=bN, bJ=bJ, bC=bC, alt_fwd=alt_fwd, alt_bwd=alt_bwd, code=code)


def link(t, g):
    """a transition passes the suffix gain if it is finite"""
    return np.where(np.isneginf(t), NEG_INF, g)


def restate_gain(t8, em, ei, en, xt, seq, m):
    """the best gain: csrc/dcp_mea.h's recursion in numpy on the matrices m of `matrices`"""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    M, L = t8.shape[1], len(seq)
    a, code = m["alt_fwd"], m["code"]
    if a == NEG_INF:
        return NEG_INF
    gM, gI = np.full((L + 6, M), NEG_INF), np.full((L + 6, M), NEG_INF)
    gN, gJ, gC = (np.full(L + 6, NEG_INF) for _ in range(3))

    def word(f, e, b, l, g):  # g + l exp(f + e + b - a) where the emission is finite
        with np.errstate(invalid="ignore"):
            s = f + e + b
            w = np.where(np.isneginf(s), 0.0, np.exp(np.where(np.isneginf(s), 0.0, s) - a))
        return np.where(np.isneginf(e), NEG_INF, g + l * w)

    gB = gPN = NEG_INF
    for j in range(L, -1, -1):
        ws = [l for l in range(1, 6) if j + l <= L]
        gP, gQ, gPN, gPJ, gPC = np.full(M, NEG_INF), np.full(M, NEG_INF), NEG_INF, NEG_INF, NEG_INF
        for l in ws:
            cd = code[j, l]
            gP = np.maximum(gP, word(m["P"][j], em[cd], m["bM"][j + l], l, gM[j + l]))
            gQ = np.maximum(gQ, word(m["Q"][j], ei[cd], m["bI"][j + l], l, gI[j + l]))
            gPN = max(gPN, float(word(m["PN"][j], en[cd], m["bN"][j + l], l, gN[j + l])))
            gPJ = max(gPJ, float(word(m["PJ"][j], en[cd], m["bJ"][j + l], l, gJ[j + l])))
            gPC = max(gPC, float(word(m["PC"][j], en[cd], m["bC"][j + l], l, gC[j + l])))
        gB = float(np.max(link(ENT, gP)))
        last = j == L
        gC[j] = max(float(link(xt[X_CT], 0.0)) if last else NEG_INF, float(link(xt[X_CC], gPC)))
        gJ[j] = max(float(link(xt[X_JB], gB)), float(link(xt[X_JJ], gPJ)))
        gN[j] = max(float(link(xt[X_NB], gB)), float(link(xt[X_NN], gPN)))
        gE = max(float(link(xt[X_ET], 0.0)) if last else NEG_INF, float(link(xt[X_EB], gB)), float(link(xt[X_EJ], gPJ)),
                 float(link(xt[X_EC], gPC)))
        gD = np.full(M + 1, NEG_INF)
        for k in range(M - 1, -1, -1):
            nx = k + 1 < M
            dn, pn = (gD[k + 1], gP[k + 1]) if nx else (NEG_INF, NEG_INF)
            t = (lambda row: row[k + 1] if nx else NEG_INF)
            gD[k] = max(gE, float(link(t(DD), dn)), float(link(t(DM), pn)))
            gM[j, k] = max(gE, float(link(t(MD), dn)), float(link(t(MM), pn)), float(link(MI[k], gQ[k])))
            gI[j, k] = max(float(link(t(IM), pn)), float(link(II[k], gQ[k])))
    return max(float(link(xt[X_SB], gB)), float(link(xt[X_SN], gPN)))


_HOST = {}


def host_case(dcp, orc, M, L, multi, eps=0.01):
    """the case's tables and the host twin's (steps, post, gain, alt_fwd); computed once"""
    key = (orc.np, M, L, multi, eps)
    if key not in _HOST:
        tabs = case(orc, M, L, multi, eps)
        _HOST[key] = tabs, dcp.mea_tables(*tabs)
    return _HOST[key]


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_against_the_restatement(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):  # float tables go in as they are: promoted to double
        (t8, em, ei, en, xt, seq), (steps, post, gain, fwd) = host_case(dcp, orc, M, L, multi)
        m = matrices(t8, em, ei, en, xt, seq)
        r = restate(t8, em, ei, en, xt, seq)  # the same operations: the same bits
        assert bits(np.array([m["alt_fwd"], m["alt_bwd"]])).tolist() == bits(np.array([r["alt_fwd"], r["alt_bwd"]])).tolist()
        want = restate_gain(t8, em, ei, en, xt, seq, m)
        n, X = emitting(steps), max(r["X"], path_x(fwd, post))
        print("host twin vs restatement M %d L %d multi %d f%d: gain %.12f, restated %.12f, gap %.3e of %.3e (%d words)" % (
            M, L, multi, 64 if orc is oracle64 else 32, gain, want, abs(gain - want), tol(2 * n, X), n))
        assert abs(gain - want) <= tol(2 * n, X)
        well_formed(steps, L)
        assert (post[steps["seqlen"] == 0] == -1.0).all() and (post[steps["seqlen"] > 0] >= 0.0).all()
        g, ps = dcp.mea_path_gain(t8, em, ei, en, xt, seq, steps)
        assert bits(np.array([g])) == bits(np.array([gain])) and np.array_equal(bits(ps), bits(post))
        assert 0.0 <= gain <= L + L * allow(X)
        assert bits(np.array([fwd])) == bits(np.array([dcp.forward_tables(t8, em, ei, en, xt, seq)[1]]))


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_the_viterbi_path_is_no_better(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):
        (t8, em, ei, en, xt, seq), (steps, post, gain, fwd) = host_case(dcp, orc, M, L, multi)
        _, al, (st, ln), _ = orc.dp_tables_path(t8, em, ei, en, xt, bytes(seq))
        if not np.isfinite(al):
            continue
        vit = as_steps(dcp, list(zip(st.tolist(), ln.tolist())))
        g, ps = dcp.mea_path_gain(t8, em, ei, en, xt, seq, vit)  # accepted: admissible
        X = max(path_x(fwd, post), path_x(fwd, ps))
        print("Viterbi path M %d L %d multi %d f%d: gain %.6f of the decoded path's %.6f" % (
            M, L, multi, 64 if orc is oracle64 else 32, g, gain))
        assert g <= gain + tol(emitting(vit) + emitting(steps), X)
        assert g <= gain  # and, both on the host's numbers, not above at all: max is exact


def test_epsilon_zero(dcp, oracle64):
    for L in (1, 7, 10):  # L mod 3 != 0: no path emits the sequence in codons alone
        t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, L, True, eps=0.0)
        steps, post, gain, fwd = dcp.mea_tables(t8, em, ei, en, xt, seq)
        assert len(steps) == 0 and len(post) == 0 and gain == NEG_INF and fwd == NEG_INF
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 9, True, eps=0.0)
    steps, post, gain, fwd = dcp.mea_tables(t8, em, ei, en, xt, seq)
    well_formed(steps, 9)
    assert np.isfinite([gain, fwd]).all() and set(steps["seqlen"][steps["seqlen"] > 0].tolist()) == {3}


def raw_tables(dcp, M, ldk, t8, em, ei, en, xt, seq, L, cap, fill=1.5, steps=True, post=True, n=True, gain=True, fwd=True):
    st, ps = np.full(max(cap, 1), 0xffff, np.uint32), np.full(max(cap, 1), fill)
    nn, g, f = C.c_uint(77), C.c_double(fill), C.c_double(fill)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = dcp.lib.dcp_mea_tables(M, ldk, P(t8), P(em), P(ei), P(en), P(xt), P(seq), L, P(st) if steps else None, cap,
                                C.byref(nn) if n else None, P(ps) if post else None,
                                C.byref(g) if gain else None, C.byref(f) if fwd else None)
    return rc, st, ps, nn.value, g.value, f.value


def test_padding_columns_change_no_bit(dcp, oracle64):
    for M, L in ((2, 7), (5, 30), (65, 60)):
        t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
        ldk = M + 7
        t8p, emp = np.full((8, ldk), NEG_INF), np.full((1364, ldk), NEG_INF)
        t8p[:, :M], emp[:, :M] = t8, em
        steps, post, gain, fwd = dcp.mea_tables(t8, em, ei, en, xt, seq)
        rc, st, ps, n, g, f = raw_tables(dcp, M, ldk, t8p, emp, ei, en, xt, seq, L, len(steps))
        assert rc == 0 and n == len(steps) and st.tobytes() == steps.tobytes()
        assert np.array_equal(bits(ps), bits(post)) and bits(np.array([g, f])).tolist() == bits(np.array([gain, fwd])).tolist()
        gg, pp = C.c_double(0.0), np.zeros(len(steps))
        assert dcp.lib.dcp_mea_path_gain(M, ldk, t8p.ctypes.data, emp.ctypes.data, ei.ctypes.data, en.ctypes.data, xt.ctypes.data,
                                         seq.ctypes.data, L, steps.ctypes.data, len(steps), C.byref(gg), pp.ctypes.data) == 0
        assert bits(np.array([gg.value])) == bits(np.array([gain])) and np.array_equal(bits(pp), bits(post))


def test_host_twin_refusals_write_nothing(dcp, oracle64):
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 30, True)
    steps, post, gain, fwd = dcp.mea_tables(t8, em, ei, en, xt, seq)
    good = dict(M=5, ldk=5, t8=t8, em=em, ei=ei, en=en, xt=xt, seq=seq, L=30)
    bad_seq = seq.copy()
    bad_seq[17] = 4
    wide = np.full((8, 4097), NEG_INF), np.full((1364, 4097), NEG_INF)
    cases = [dict(M=0), dict(M=4097, ldk=4097, t8=wide[0], em=wide[1]), dict(ldk=4), dict(L=0), dict(seq=bad_seq),
             dict(t8=None), dict(em=None), dict(ei=None), dict(en=None), dict(xt=None), dict(seq=None)]

    def untouched(st, ps, n, g, f, count=77):
        return (st == 0xffff).all() and (ps == 1.5).all() and n == count and g == 1.5 and f == 1.5

    for change in cases:
        a = dict(good, **change)
        rc, *out = raw_tables(dcp, a["M"], a["ldk"], a["t8"], a["em"], a["ei"], a["en"], a["xt"], a["seq"], a["L"], len(steps))
        assert rc == dcp.RC_EINVAL and untouched(*out), change
    for missing in ("steps", "post", "n", "gain", "fwd"):
        rc, *out = raw_tables(dcp, 5, 5, t8, em, ei, en, xt, seq, 30, len(steps), **{missing: False})
        assert rc == dcp.RC_EINVAL and untouched(*out), missing
    # one step short: the count, and nothing else
    rc, *out = raw_tables(dcp, 5, 5, t8, em, ei, en, xt, seq, 30, len(steps) - 1)
    assert rc == dcp.RC_ENOMEM and untouched(*out, count=len(steps))
    rc, st, ps, n, g, f = raw_tables(dcp, 5, 5, t8, em, ei, en, xt, seq, 30, len(steps))
    assert rc == 0 and n == len(steps) and st.tobytes() == steps.tobytes()
    with pytest.raises(dcp.DcpError):
        dcp.mea_tables(t8, em[:, :4], ei, en, xt, seq)

    # mea_path_gain
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def raw_gain(st, a=good, gain=True):
        g, ps = C.c_double(1.5), np.full(max(len(st), 1) if st is not None else 1, 1.5)
        rc = dcp.lib.dcp_mea_path_gain(a["M"], a["ldk"], P(a["t8"]), P(a["em"]), P(a["ei"]), P(a["en"]), P(a["xt"]), P(a["seq"]),
                                       a["L"], P(st), 0 if st is None else len(st), C.byref(g) if gain else None, P(ps))
        return rc, g.value == 1.5 and (ps == 1.5).all()

    assert raw_gain(steps)[0] == 0
    for change in cases:
        assert raw_gain(steps, dict(good, **change)) == (dcp.RC_EINVAL, True), change
    assert raw_gain(steps, gain=False) == (dcp.RC_EINVAL, True)
    pairs = list(zip(steps["state_id"].tolist(), steps["seqlen"].tolist()))
    first_m = next(i for i, (sid, l) in enumerate(pairs) if sid >> 14 == 0)
    sid, l = pairs[first_m]
    off_graph = pairs[:first_m] + [(sid, l), (((sid & 0x3fff) + 2) if (sid & 0x3fff) + 2 <= 5 else 1, 0)] + pairs[first_m + 1:]
    off_graph[first_m + 1] = (off_graph[first_m + 1][0], 0)
    emitter = max(i for i, (_, l) in enumerate(pairs) if l > 1)
    short = list(pairs)
    short[emitter] = (short[emitter][0], short[emitter][1] - 1)  # emits L - 1
    node = list(pairs)
    node[first_m] = (6, l)  # node M + 1
    no_s, no_t = pairs[1:], pairs[:-1]
    for what, bad in (("an edge out of the graph", off_graph), ("L - 1 bases", short), ("node M + 1", node), ("no S", no_s),
                      ("no T", no_t), ("one step", pairs[:1])):
        assert raw_gain(as_steps(dcp, bad)) == (dcp.RC_EINVAL, True), what
    assert raw_gain(None) == (dcp.RC_EINVAL, True)  # a null path
    assert raw_gain(np.zeros(0, dcp.STEP_DTYPE)) == (dcp.RC_EINVAL, True)
    with pytest.raises(dcp.DcpError):
        dcp.mea_path_gain(t8, em, ei, en, xt, seq, as_steps(dcp, short))
    # not admissible: the path's own edge made -inf
    k = (sid & 0x3fff) - 1
    shut = t8.copy()
    shut[0, k] = NEG_INF  # entry_k
    if pairs[first_m - 1][0] == B_:
        assert raw_gain(steps, dict(good, t8=shut)) == (dcp.RC_EINVAL, True)


def test_mea_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_mea.c with the host model alone (no device code) under ASan + UBSan, as a program of its own."""
    obj, exe = str(tmp_path / "asan_mea.o"), str(tmp_path / "asan_mea")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_mea.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_mea ok" in r.stdout


# ---- GPU: the device against the host twin ----------------------------------------------------------------------------
_REF = {}


def reference(dcp, precision, orc64):
    """per flags and (q, p): the host twin's (steps, post, gain, alt_fwd) on the tables the device holds; computed once"""
    if precision not in _REF:
        profs, seqs, tabs = world(dcp, precision, orc64)[:3]
        ref = {}
        for multi, h3 in FLAGS:
            for q, s in enumerate(seqs):
                xt = xtrans_of(dcp, precision, len(s), multi, h3)
                for p in range(len(profs)):
                    ref[multi, h3, q, p] = dcp.mea_tables(*tabs[p], xt, s)
        _REF[precision] = ref
    return _REF[precision]


def check_against(dcp, res, cases, what):
    """every pair of mea_pairs' result against its (tables, xt, seq, host twin's result): the device's path is admissible
    and emits L on the host's tables, its host-evaluated gain lies within the tolerance below the host's optimum and not
    above it, gain_out and the posteriors lie within theirs of the host's for that path; no path where the host has
    none.  Returns the worst ratios (shortfall / tolerance, gain_out / tolerance, posterior / allow)."""
    paths, posts, gain, fwd = res
    assert len(paths) == len(posts) == len(gain) == len(fwd) == len(cases)
    w_short = w_gain = w_post = 0.0
    for i, (tabs, xt, seq, (hsteps, hpost, hgain, hfwd)) in enumerate(cases):
        assert paths[i].dtype == dcp.STEP_DTYPE and posts[i].dtype == np.float64 and len(paths[i]) == len(posts[i])
        assert within([fwd[i]], [hfwd]), (what, i)
        if hfwd == NEG_INF:
            assert len(paths[i]) == 0 and gain[i] == NEG_INF, (what, i)
            continue
        well_formed(paths[i], len(seq))
        g, ps = dcp.mea_path_gain(*tabs, xt, seq, paths[i])  # accepted: admissible, emits L
        n_dev, n_host = emitting(paths[i]), emitting(hsteps)
        X = max(path_x(hfwd, hpost), path_x(hfwd, ps))
        assert g <= hgain, (what, i, g, hgain)
        assert hgain - g <= tol(n_dev + n_host, X), (what, i, hgain, g, tol(n_dev + n_host, X))
        assert abs(gain[i] - g) <= tol(n_dev, X), (what, i, gain[i], g)
        silent = paths[i]["seqlen"] == 0
        assert (posts[i][silent] == -1.0).all() and (ps[silent] == -1.0).all()
        d = float(np.max(np.abs(posts[i][~silent] - ps[~silent])))
        assert d <= allow(X), (what, i, d, allow(X))
        w_short = max(w_short, (hgain - g) / tol(n_dev + n_host, X))
        w_gain, w_post = max(w_gain, abs(gain[i] - g) / tol(n_dev, X)), max(w_post, d / allow(X))
    return w_short, w_gain, w_post


def same_result(x, y):
    return (all(a.tobytes() == b.tobytes() for a, b in zip(x[0], y[0])) and
            all(np.array_equal(bits(a), bits(b)) for a, b in zip(x[1], y[1])) and
            np.array_equal(bits(x[2]), bits(y[2])) and np.array_equal(bits(x[3]), bits(y[3])) and len(x[0]) == len(y[0]))


def world_cases(dcp, precision, orc64, sq, pr, multi=True, h3=False):
    profs, seqs, tabs = world(dcp, precision, orc64)[:3]
    ref = reference(dcp, precision, orc64)
    return [(tabs[p], xtrans_of(dcp, precision, len(seqs[q]), multi, h3), seqs[q], ref[multi, h3, q, p]) for q, p in zip(sq, pr)]


_EVERY = {}


def every_pair(dcp, precision, orc64, multi, h3):
    """mea_pairs and forward_pairs of all pairs of the world, shuffled; run once per flags"""
    key = (precision, multi, h3)
    if key not in _EVERY:
        profs, seqs = world(dcp, precision, orc64)[:2]
        every = [(q, p) for q in range(len(seqs)) for p in range(len(profs))]
        order = np.random.default_rng(14).permutation(len(every))
        sq, pr = np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])
        sc = loaded(dcp, precision)
        res = sc.mea_pairs(sq, pr, multi, h3)
        ms = sc.mea_kernel_ms
        alt = sc.forward_pairs(sq, pr, multi, h3)[1]
        sc.close()
        _EVERY[key] = sq, pr, res, alt, ms
    return _EVERY[key]


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pair_against_the_host_twin(dcp, oracle64, precision, multi, h3):
    sq, pr, res, alt, ms = every_pair(dcp, precision, oracle64, multi, h3)
    assert ms > 0
    assert np.array_equal(bits(res[3]), bits(alt))  # one sweep: the bits of forward_pairs
    ratios = check_against(dcp, res, world_cases(dcp, precision, oracle64, sq, pr, multi, h3), (precision, multi, h3))
    print("device vs host twin f%d multi %d h3 %d: shortfall %.3e of its tolerance, gain_out %.3e of its, posteriors %.3e of "
          "allow" % ((precision, multi, h3) + ratios))
    assert np.isfinite(res[3]).sum() > len(sq) // 2
    for path, a, g in zip(res[0], res[3], res[2]):
        assert (len(path) == 0) == (a == NEG_INF) == (g == NEG_INF)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_few_wavefronts_and_a_small_budget_change_no_bit(dcp, oracle64, precision):
    """the stride loop's second trip, a wide pair behind a narrower one in the same work area; rounds of a few pairs, of one
    pair, a pair larger than the budget in a round of its own"""
    profs, seqs = world(dcp, precision, oracle64)[:2]
    ix = {M: i for i, M in enumerate(WORLD_M)}
    q = WORLD_L.index(100)
    pairs = [(q, ix[1100]), (q, ix[257]), (q, ix[1100]), (q, ix[2]), (q, ix[513])]
    pairs += [(8, ix[512]), (7, ix[64]), (8, ix[129]), (5, ix[1100]), (8, len(WORLD_M)), (6, ix[256]), (0, ix[63]), (3, ix[128])]
    sq, pr = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    sc = loaded(dcp, precision, dcp.load_testhooks())
    base = sc.mea_pairs(sq, pr)
    check_against(dcp, base, world_cases(dcp, precision, oracle64, sq, pr), precision)
    for cap in (3, 1, 0):
        sc.test_set_forward_waves(cap)
        assert same_result(sc.mea_pairs(sq, pr), base), cap
    # 34 bytes a cell: a few pairs a round, one 100-nt pair of 257 nodes a round, every pair alone
    for budget in (34 * 101 * 1400, 34 * 101 * 257 + 88 * 101, 1, 0):
        sc.test_set_mea_budget(budget)
        assert same_result(sc.mea_pairs(sq, pr), base), budget
    sc.test_set_mea_budget(34 * 101 * 1400)
    sc.test_set_forward_waves(1)
    assert same_result(sc.mea_pairs(sq, pr), base)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lists_come_back_in_list_order(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    sc = loaded(dcp, precision)
    assert sc.mea_kernel_ms < 0  # none has run
    paths, posts, gain, fwd = sc.mea_pairs([], [])
    assert paths == [] and posts == [] and gain.shape == fwd.shape == (0,)
    assert sc.mea_kernel_ms < 0 and sc.forward_kernel_ms < 0 and sc.posterior_kernel_ms < 0
    res = sc.mea_pairs([8], [9])
    check_against(dcp, res, world_cases(dcp, precision, oracle64, [8], [9]), precision)
    assert sc.mea_kernel_ms > 0 and sc.forward_kernel_ms < 0 and sc.posterior_kernel_ms < 0  # their clocks are their own
    sq, pr = np.array([7, 8, 7, 7, 3, 8]), np.array([11, 4, 11, 11, 0, 4])
    res = sc.mea_pairs(sq, pr)
    check_against(dcp, res, world_cases(dcp, precision, oracle64, sq, pr), precision)
    for i, j in ((0, 2), (0, 3), (1, 5)):  # listed twice: decoded twice
        assert res[0][i].tobytes() == res[0][j].tobytes() and np.array_equal(bits(res[1][i]), bits(res[1][j]))
        assert bits(res[2])[i] == bits(res[2])[j] and bits(res[3])[i] == bits(res[3])[j]
    # step_off is cumulative
    off = np.full(len(sq) + 1, 7, np.uint32)
    n = sum(len(p) for p in res[0])
    steps, post, gain, fwd = np.zeros(n, dcp.STEP_DTYPE), np.zeros(n), np.zeros(len(sq)), np.zeros(len(sq))
    s32, p32 = sq.astype(np.uint32), pr.astype(np.uint32)
    assert sc._lib.dcp_gpu_mea_pairs(sc._c, 1, 0, s32.ctypes.data, p32.ctypes.data, len(sq), steps.ctypes.data, n, off.ctypes.data,
                                     post.ctypes.data, gain.ctypes.data, fwd.ctypes.data) == 0
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in res[0]])]).tolist()
    assert steps.tobytes() == np.concatenate(res[0]).tobytes()
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_batches(dcp, oracle64, precision):
    profs, seqs, tabs = world(dcp, precision, oracle64)[:3]
    ref = reference(dcp, precision, oracle64)
    eps0 = dcp.ProteinProfile.sample(77, 70, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    mine = [profs[3], eps0, profs[8], profs[12]]
    sc = dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs(seqs)
    mytabs = device_tables(dcp, sc, mine, precision, 0.0)[1]
    sq, pr = np.arange(len(seqs)).repeat(4), np.tile(np.arange(4), len(seqs))
    res = sc.mea_pairs(sq, pr)
    sc.close()
    cases = []
    for q, s in enumerate(seqs):
        xt = xtrans_of(dcp, precision, len(s), True, False)
        cases += [(tabs[3], xt, s, ref[True, False, q, 3]), (mytabs, xt, s, dcp.mea_tables(*mytabs, xt, s)),
                  (tabs[8], xt, s, ref[True, False, q, 8]), (tabs[12], xt, s, ref[True, False, q, 12])]
        mine_q = res[0][4 * q + 1]
        if len(s) % 3:  # epsilon 0: no path emits the sequence in codons alone
            assert len(mine_q) == 0 and res[2][4 * q + 1] == NEG_INF and res[3][4 * q + 1] == NEG_INF
        elif len(mine_q):  # (a stop codon in every frame leaves none either)
            assert set(mine_q["seqlen"][mine_q["seqlen"] > 0].tolist()) == {3}
    check_against(dcp, res, cases, (precision, "eps0"))

    def twin_case(p, xt, s):
        return tabs[p], xt, s, dcp.mea_tables(*tabs[p], xt, s)

    # both strands: resident n + q is the reverse complement of q
    sc = loaded(dcp, precision)
    n = len(seqs)
    sc.add_reverse_strand()
    sq, pr = np.array([n + 8, n + 7, 8, n + 5]), np.array([9, 12, 9, 2])
    res = sc.mea_pairs(sq, pr)
    sc.close()
    cases = [twin_case(p, xtrans_of(dcp, precision, len(seqs[q % n]), True, False),
                       np_revcomp(seqs[q % n]) if q >= n else seqs[q % n]) for q, p in zip(sq, pr)]
    check_against(dcp, res, cases, (precision, "strands"))

    # regions cut out of the batch
    sc = loaded(dcp, precision)
    sc.cut_regions([8, 8, 7], [0, 100, 30], [333, 150, 64], [0, 1, 0])
    sq, pr = np.array([0, 1, 2, 1]), np.array([10, 6, 12, 0])
    cut = [seqs[8], np_revcomp(seqs[8][100:250]), seqs[7][30:94]]
    res = sc.mea_pairs(sq, pr)
    sc.close()
    cases = [twin_case(p, xtrans_of(dcp, precision, len(cut[q]), True, False), cut[q]) for q, p in zip(sq, pr)]
    check_against(dcp, res, cases, (precision, "regions"))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_transitions_in_the_dbs_precision(dcp, oracle64, precision):
    profs, seqs, tabs = world(dcp, precision, oracle64)[:3]
    ref = reference(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    sq, pr = np.array([8, 7, 4, 8, 2]), np.array([12, 9, 5, 11, 1])
    res = sc.mea_pairs(sq, pr, True, False)  # the flags are ignored
    check_against(dcp, res, [(tabs[p], xt[q], seqs[q], dcp.mea_tables(*tabs[p], xt[q], seqs[q])) for q, p in zip(sq, pr)], precision)
    assert not within(res[3], [ref[True, False, q, p][3] for q, p in zip(sq, pr)])
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.mea_pairs(sq, pr))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_and_capacity_leave_the_outputs(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.mea_pairs([0], [0]))  # no DB
    sc.upload_db(profs)
    refused(dcp, sc, lambda: sc.mea_pairs([0], [0]))  # no batch
    sc.upload_seqs(seqs)
    with pytest.raises(dcp.DcpError) as e:
        sc.mea_pairs([0, len(seqs), 99], [0, 0, 99])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    with pytest.raises(dcp.DcpError) as e:
        sc.mea_pairs([0, 1], [0, len(profs)])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    refused(dcp, sc, lambda: sc.mea_pairs([0, 1], [0]))
    sq, pr = np.array([8, 5], np.uint32), np.array([0, 3], np.uint32)
    want = sc.mea_pairs(sq, pr)
    need = sum(len(p) for p in want[0])
    off = np.full(3, 7, np.uint32)
    steps, post = np.full(need, 0xffff, np.uint32), np.full(need, 1.5)
    gain, fwd = np.full(2, 2.5), np.full(2, 2.5)
    call = sc._lib.dcp_gpu_mea_pairs
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def run(sq_=sq, pr_=pr, steps_=steps, cap=need, off_=off, post_=post, gain_=gain, fwd_=fwd, n=2):
        return call(sc._c, 1, 0, P(sq_), P(pr_), n, P(steps_), cap, P(off_), P(post_), P(gain_), P(fwd_))

    def untouched(offsets=True):
        return ((not offsets or off.tolist() == [7, 7, 7]) and (steps == 0xffff).all() and (post == 1.5).all() and
                (gain == 2.5).all() and (fwd == 2.5).all())

    for change in (dict(sq_=None), dict(pr_=None), dict(steps_=None), dict(off_=None), dict(gain_=None), dict(fwd_=None),
                   dict(sq_=np.array([8, 99], np.uint32))):
        assert run(**change) == dcp.RC_EINVAL and untouched(), change
        assert len(sc._lib.dcp_gpu_last_error(sc._c)) > 0
    # capacity one short: step_off names the need, nothing else is written
    assert run(cap=need - 1) == dcp.RC_ENOMEM and untouched(offsets=False)
    assert off.tolist() == [0, len(want[0][0]), need] and str(need) in sc._lib.dcp_gpu_last_error(sc._c).decode()
    assert run() == 0
    assert steps.tobytes() == np.concatenate(want[0]).tobytes() and np.array_equal(bits(gain), bits(want[2]))
    assert np.array_equal(bits(post), bits(np.concatenate(want[1])))
    steps[:] = 0xffff
    assert run(post_=None) == 0 and steps.tobytes() == np.concatenate(want[0]).tobytes()  # post_out may be NULL
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_else_moves(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    sc = loaded(dcp, precision)
    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    nl, al = sc.scores()
    hits, cells, launches = sc.hits().copy(), sc.cells, sc.last_scan_launches
    assert len(hits) > 0
    sq, pr = np.array([8, 7, 6, 8]), np.array([11, 3, 0, 12])
    f0, p0 = sc.forward_pairs(sq, pr, False, False), sc.posterior_pairs(sq, pr, False, False)
    res = sc.mea_pairs(sq, pr, False, False)  # other flags than the scan's
    check_against(dcp, res, world_cases(dcp, precision, oracle64, sq, pr, False, False), precision)
    f1, p1 = sc.forward_pairs(sq, pr, False, False), sc.posterior_pairs(sq, pr, False, False)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(f0, f1))
    assert np.array_equal(p0[0], p1[0]) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(p0[1:], p1[1:]))
    assert np.array_equal(bits(res[3]), bits(f0[1]))
    n2, a2 = sc.scores()
    assert np.array_equal(bits(n2), bits(nl)) and np.array_equal(bits(a2), bits(al))
    assert sc.hits().tobytes() == hits.tobytes() and sc.cells == cells and sc.last_scan_launches == launches
    sc.close()


def pair_records(dcp, precision, sq, pr):
    """hit records that name the pairs, for the calls that take paths"""
    hits = np.zeros(len(sq), dcp.HIT64_DTYPE if precision == 64 else dcp.HIT_DTYPE)
    hits["seq_idx"], hits["profile_idx"] = sq, pr
    return hits


def path_total(tabs, xt, seq, steps):
    """path_domains' total of a path -- every transition and every emission along it, in step order -- summed in double
    on the given tables; -inf if an edge is not in the graph"""
    t8, em, ei, en = (np.asarray(a, np.float64) for a in tabs)
    xt = np.asarray(xt, np.float64)
    special = {(S_, N_): X_SN, (N_, N_): X_NN, (S_, B_): X_SB, (N_, B_): X_NB, (E_, B_): X_EB, (J_, B_): X_JB, (E_, J_): X_EJ,
               (J_, J_): X_JJ, (E_, C_): X_EC, (C_, C_): X_CC, (E_, T_): X_ET, (C_, T_): X_CT}
    total, pos, prev = 0.0, 0, None
    for sid, l in zip(steps["state_id"].tolist(), steps["seqlen"].tolist()):
        kind, k = sid >> 14, (sid & 0x3fff) - 1
        if prev is not None:
            pkind, pk = prev >> 14, (prev & 0x3fff) - 1
            if kind == 3:
                t = 0.0 if sid == E_ and pkind in (0, 2) else xt[special[prev, sid]] if (prev, sid) in special else NEG_INF
            elif kind == 0:  # M_k: from B, or from M, I, D of node k - 1
                t = t8[0, k] if prev == B_ else t8[1 + pkind, k] if pkind < 3 and pk == k - 1 else NEG_INF
            elif kind == 1:  # I_k: from M_k or itself
                t = t8[6 + pkind, k] if pkind < 2 and pk == k else NEG_INF
            else:  # D_k: from M or D of node k - 1
                t = t8[4 if pkind == 0 else 5, k] if pkind in (0, 2) and pk == k - 1 else NEG_INF
            total = total + float(t)
        if l:
            code = word_code(seq, pos, l)
            total = total + float(em[code, k] if kind == 0 else ei[code] if kind == 1 else en[code])
        pos, prev = pos + l, sid
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_downstream_takes_the_paths(dcp, oracle64, precision):
    """path_domains and decode_paths take the decoded paths as they are.  Every path's total is finite; summed in double
    on the tables the device holds it is at most the pair's Viterbi score in double on the same tables plus the score
    allowance, 2^-32 (|x| + 1); so is path_domains' own total on a double DB.  On a float DB path_domains sums in float,
    which no bound in double holds (seen: 3.3e-5 above the double Viterbi score where both paths are the same path): that
    total is held to be finite, no more."""
    profs, seqs, tabs, _, _, vit = world(dcp, precision, oracle64)
    sq, pr, res, alt, ms = every_pair(dcp, precision, oracle64, True, False)
    keep = [i for i in range(len(sq)) if len(res[0][i])]
    paths = [res[0][i] for i in keep]
    hits = pair_records(dcp, precision, sq[keep], pr[keep])
    sc = dcp.Scanner(0)
    sc.keep_dists(True)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    domains, dom_off, core, null, total = sc.path_domains(hits, paths, True, False)
    codes = sc.decode_paths(hits, paths)
    sc.close()
    total = np.asarray(total, np.float64)
    assert len(total) == len(keep) and np.isfinite(total).all()
    assert all(dom_off[i + 1] > dom_off[i] for i in range(len(keep)))  # every alt path holds a domain
    va = vit[True, False][1][sq[keep], pr[keep]]
    host = np.array([path_total(tabs[p], xtrans_of(dcp, precision, len(seqs[q]), True, False), seqs[q], path)
                     for q, p, path in zip(sq[keep], pr[keep], paths)])
    allowance = 2.0 ** -32 * (np.abs(va) + 1.0)
    print("path totals f%d: in double closest to the Viterbi score %.3e below it; path_domains' own %.3e; the two apart by "
          "%.3e of (|x| + 1) at most" % (precision, float(np.min(va - host)), float(np.min(va - total)),
                                         float(np.max(np.abs(total - host) / (np.abs(host) + 1.0)))))
    assert np.isfinite(host).all() and np.isfinite(va).all()
    assert (host <= va + allowance).all()  # a path weighs at most the best path
    if precision == 64:
        assert (total <= va + allowance).all()
        assert (np.abs(total - host) <= allowance).all()
    assert [len(c) for c in codes] == [len(p) for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_planted_gene_and_the_viterbi_paths(dcp, oracle32, oracle64, precision):
    """the 333-nt query of tests/test_scan_pairs.py carries the 64-node profile's gene in bases [70, 262): a domain of the
    decoded path overlaps it; and the Viterbi paths of trace_paths have, on the host's numbers, at most the device's gain"""
    from test_scan_pairs import pair_world
    profs, seqs = pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)[:2]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    paths, posts, gain, fwd = sc.mea_pairs([5], [1])
    doms = sc.path_domains(pair_records(dcp, precision, [5], [1]), paths, True, False)[0]
    sc.close()
    overlap = sum(max(0, min(int(d["seq_end"]), 262) - max(int(d["seq_begin"]), 70)) for d in doms)
    print("planted gene [70, 262) f%d: %d domains, overlap %d bases, gain %.3f" % (precision, len(doms), overlap, gain[0]))
    assert overlap > 0

    profs, seqs, tabs = world(dcp, precision, oracle64)[:3]
    sq, pr = np.array([8, 7, 6, 8, 4], np.uint32), np.array([11, 3, 0, 12, 9], np.uint32)
    sc = loaded(dcp, precision)
    res = sc.mea_pairs(sq, pr)
    vpaths = sc.trace_paths(pair_records(dcp, precision, sq, pr), True, False)[0]
    sc.close()
    for i, (q, p) in enumerate(zip(sq, pr)):
        xt = xtrans_of(dcp, precision, len(seqs[q]), True, False)
        gv, pv = dcp.mea_path_gain(*tabs[p], xt, seqs[q], vpaths[i])
        gd, pd = dcp.mea_path_gain(*tabs[p], xt, seqs[q], res[0][i])
        X = max(path_x(res[3][i], pv), path_x(res[3][i], pd))
        assert abs(res[2][i] - gd) <= tol(emitting(res[0][i]), X)  # gain_out is the device's own number for its path
        assert gv <= gd + tol(emitting(vpaths[i]) + emitting(res[0][i]), X)  # both on the host's numbers


_CHAIN = {}


def chain_mea_world(dcp, oracle64, precision):
    """The delete-heavy and severed profiles of tests/test_forward_chain_edges.py's chain_world with queries that skip
    nodes: the best codons of nodes a .. a + 3 and a + 36 .. a + 39 of a profile, a = 0 for every width and a = 238 for the
    wide ones (the run of 32 deletes in between then crosses column 256, a chunk's edge and the severed profiles' cut).
    In uni-hit mode the decoded path of such a query against its own profile can join the two stretches of match words
    only through D steps (in multi-hit mode E -> B joins them at the same gain, and E comes first).  Per flags and (q, p)
    the host twin on the tables the device holds; computed once."""
    if precision not in _CHAIN:
        import test_forward_chain_premises as prem
        from test_forward_chain_edges import chain_world
        from test_trace_oracle import best_codons
        specs, profs = chain_world(dcp, precision)[:2]
        ix = [i for i, s in enumerate(specs) if s[0] in ("delete", "severed")]
        seqs = []
        for M in sorted({specs[i][1] for i in ix}):
            op = oracle64.new(*prem.chain_params("delete", M), ENTRY_DIST_OCCUPANCY, prem.EPS)
            for a in (0, 238) if M >= 513 else (0,):
                seqs.append(np.frombuffer(best_codons(op, list(range(a, a + 4)) + list(range(a + 36, a + 40))), np.uint8).copy())
        mine = [profs[i] for i in ix]
        sc = dcp.Scanner(0)
        sc.upload_db(mine)
        sc.upload_seqs(seqs)
        tabs = device_tables(dcp, sc, mine, precision, prem.EPS)
        sc.close()
        ref = {}
        for multi in (False, True):
            for q, s in enumerate(seqs):
                xt = xtrans_of(dcp, precision, len(s), multi, False)
                for p in range(len(mine)):
                    ref[multi, q, p] = dcp.mea_tables(*tabs[p], xt, s)
        _CHAIN[precision] = [specs[i] for i in ix], mine, seqs, tabs, ref
    return _CHAIN[precision]


def delete_steps(path):
    return int(np.count_nonzero(path["state_id"] >> 14 == 2))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_delete_chain(dcp, oracle64, precision):
    specs, profs, seqs, tabs, ref = chain_mea_world(dcp, oracle64, precision)
    # a condition on the inputs: in either family a decoded path of the host twin holds D steps
    for fam in ("delete", "severed"):
        runs = [delete_steps(ref[False, q, p][0]) for q in range(len(seqs)) for p in range(len(profs)) if specs[p][0] == fam]
        print("host twin f%d %s: %d of %d uni-hit paths hold D steps, the longest run of them %d" % (
            precision, fam, sum(r > 0 for r in runs), len(runs), max(runs)))
        assert max(runs) >= 32
    every = [(q, p) for q in range(len(seqs)) for p in range(len(profs))]
    order = np.random.default_rng(15).permutation(len(every))
    sq, pr = np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    for multi in (False, True):
        res = sc.mea_pairs(sq, pr, multi, False)
        cases = [(tabs[p], xtrans_of(dcp, precision, len(seqs[q]), multi, False), seqs[q], ref[multi, q, p]) for q, p in zip(sq, pr)]
        ratios = check_against(dcp, res, cases, (precision, multi))
        nd = [delete_steps(p) for p in res[0]]
        print("device vs host twin f%d chain world multi %d: shortfall %.3e of its tolerance, gain_out %.3e of its, posteriors "
              "%.3e of allow; %d paths hold D steps, %d of them at most" % ((precision, multi) + ratios + (sum(n > 0 for n in nd), max(nd))))
        if not multi:
            for fam in ("delete", "severed"):
                assert max(n for n, p in zip(nd, pr) if specs[p][0] == fam) >= 32
    sc.close()
