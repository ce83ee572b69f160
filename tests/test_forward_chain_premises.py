"""The worlds of tests/test_forward_chain_edges.py -- Forward and Backward sweeps where the delete chain carries weight
-- and what they rest on, checked on the CPU.

forward_kernel / forward_wide_kernel (csrc/dcp_forward.hip) and backward_kernel / backward_wide_kernel
(csrc/dcp_posterior.hip) close the in-row delete chain by a scan over the 64 lanes: a lane's R nodes compose to the map
d_out = lse(c, d_in + s), the maps are composed inclusively in six steps (o = 1, 2, .., 32), the composed map of the
lanes before is applied to the carry of the chunk before, and the lane's chain is run again from its true input
(DESIGN sections 19 and 20).  In the world of tests/test_forward_pairs.py (pfam_like_params: MD = log 0.025,
DD = log 0.4) a delete run of n nodes weighs 0.4^n: what the far scan steps and the chunk carry bring in lies below the
GPU tests' allowance of 2^-32 (|x| + 1), so a wrong lane guard, a wrong s sum, a wrong identity at lane 0 / lane 63 or
a wrong carry composition there would pass.  The worlds below are built so that it could not:

  delete-heavy    delete_heavy_params of tests/test_gpu_parity.py (MD = log 0.65, DD = log 0.92) at 64, 128, 256 nodes
                  (a full class R = 1, 2, 4: lane 63 is real), 257, 513, 1100 and 4096 (the maximum: 16 chunks)
  positive chain  pfam-like with MD = +0.7, DD = +0.4 on nodes 1 .. M - 1 at 64, 256, 600 nodes: the delete run outweighs
                  everything, s sums to a few hundred
  severed chain   delete-heavy with DD_k = MD_k = -inf at one node k: k = 32 R (a lane boundary in the middle of the
                  wave) and k = 64 R - 1 (inside lane 63) for R = 1, 2, 4; k = 256 and k = 512 (each chunk's first
                  column) for 513 and 1100 nodes.  s is -inf in a lane; nothing may become NaN
  epsilon 0       delete-heavy at 64 and 600 nodes with epsilon 0: where L mod 3 != 0 every E term of every row, in every
                  chunk of the running form, is -inf
  queries         random, L = 1, 6, 12, 40: rows 1 .. 5 with the short words, one trip of the loop unrolled by five, several

What is asserted here, with a numpy restatement of the chain AS THE DEVICE LAYS IT OUT (columns padded to chunks of 64 R,
the lanes' maps, the inclusive scan, the carry; its mirror for Backward) inside a Forward and a Backward restatement, on
the oracle's f64 tables, multi-hit:

  premise 0  with nothing knocked out the emulation equals the plain restatements (restate of test_forward_pairs.py
             with Lse, restate of test_posterior_pairs.py) within 2^-45 (|x| + 1), and the host twins -- the GPU file's
             reference -- lie within its allowance of the emulation
  premise 1  on the delete-heavy tables of 64, 128, 256, 513, 1100 nodes (L = 12; 6 for 1100) each of the six scan steps
             left out moves the alt score by at least BOUND = 2^-26 (|x| + 1), 64 times the GPU allowance; so does each
             chunk carry cut (wide profiles): Forward ed_ (D of the chunk's last node), em_ (its M, for the next node's
             M -> D) and the second pass's bm / bi / bd, each alone and the three together; Backward the carried bD and
             the carried bP.  One exception in shape, not in bound: bi alone (an insert at a chunk's edge) weighs 2^-36.9
             in the 6 rows of the 1100-node case, and is asserted for it at 12 rows
  premise 2  the positive-chain profiles meet BOUND for step o = 32, both sweeps
  premise 3  every severed profile's scores differ from the unsevered profile's by more than BOUND: the cut lies in the
             part that carries weight
  and the same knock-outs in the pfam-like world are printed, not asserted: the gap these files close.

So a kernel with one of these knock-outs as its bug moves a score of tests/test_forward_chain_edges.py by at least 64
times what that file allows, and could not pass it.  Measured minima of |delta| / (|x| + 1) over the asserted
knock-outs (this file prints every figure):

  premise 1, scan steps      Forward 2^-23.6, Backward 2^-25.9 (both: 1100 nodes x 6 nt, o = 32; at the other four sizes
                             2^-21.2 at the least, o = 32 of 513 nodes)
  premise 1, chunk carries   Forward: ed 2^-10.3, em 2^-15.0, bm 2^-19.0, bd 2^-15.7, the three together 2^-15.4, bi alone
                             2^-24.3 (1100 nodes x 12 nt);  Backward: bD 2^-10.3, bP 2^-15.4
  premise 2, o = 32          Forward 2^-1.1, Backward 2^-1.2 (600 nodes)
  premise 3                  2^-13.5, both sweeps (513 nodes severed at 512)
  pfam-like (printed)        o = 32 moves the score by 2^-52.6 at 64 nodes and by no bit from 128 nodes on; o = 16 by
                             2^-34.8 at 64 nodes and 2^-52.5 or nothing beyond; o = 8 by 2^-36.8 at 128 nodes and no bit from 256 on; o = 4 by 2^-34.7
                             or less from 256 nodes on
"""
import math

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_forward_pairs import CODE_OFF, Lse
from test_forward_pairs import restate as forward_plain
from test_gpu_parity import delete_heavy_params, pfam_like_params
from test_posterior_pairs import restate as both_plain

NEG_INF = float("-inf")
BOUND = 2.0 ** -26  # 64 times the GPU allowance of 2^-32
EQUAL = 2.0 ** -45
EPS = float(np.float32(0.01))
WIDE_CHUNK = 256
STEPS = (1, 2, 4, 8, 16, 32)
FWD_CUTS = ("ed", "em", "bm", "bi", "bd", "bm+bi+bd")
BWD_CUTS = ("bD", "bP")

# ---- the worlds: one definition for this file and tests/test_forward_chain_edges.py ---------------------------------
QUERY_L = (1, 6, 12, 40)
DELETE_M = (64, 128, 256, 257, 513, 1100, 4096)
POSITIVE_M = (64, 256, 600)
SEVERED = ((64, 32), (64, 63), (128, 64), (128, 127), (256, 128), (256, 255), (513, 256), (513, 512), (1100, 256),
           (1100, 512))  # (M, k)
EPS0_M = (64, 600)
PREMISE_SHAPES = ((64, 12), (128, 12), (256, 12), (513, 12), (1100, 6))  # (M, L): the Python loops stay within seconds


def nodes_per_lane(M):
    """R of the register classes; 0: the wide kernels (chunks of 256 columns, four nodes per lane)"""
    return 1 if M <= 64 else 2 if M <= 128 else 4 if M <= 256 else 0


def chunk_of(M):
    return 64 * nodes_per_lane(M) or WIDE_CHUNK


def chain_params(family, M, k=None):
    """(null, match, trans) of from_params; a severed profile shares everything but node k with the delete-heavy one"""
    rng = np.random.default_rng(7000 + M)
    if family in ("pfam", "positive"):
        null, match, trans = pfam_like_params(rng, M)
        if family == "positive":  # the construction of tests/test_forward_pairs.py's 90-node profile
            trans = trans.copy()
            trans[1:M, 2] = np.float32(0.7)
            trans[1:M, 6] = np.float32(0.4)
        return null, match, trans
    null, match, trans = delete_heavy_params(rng, M)
    if family == "severed":
        trans = trans.copy()
        trans[k, 2] = trans[k, 6] = -np.inf  # MD_k, DD_k: no delete state at node k
    else:
        assert family in ("delete", "eps0") and k is None
    return null, match, trans


def world_specs():
    """[(family, M, k, epsilon)] in the order of the DB"""
    return ([("delete", M, None, EPS) for M in DELETE_M] + [("positive", M, None, EPS) for M in POSITIVE_M] +
            [("severed", M, k, EPS) for M, k in SEVERED] + [("eps0", M, None, 0.0) for M in EPS0_M])


def world_queries():
    rng = np.random.default_rng(7)
    return [rng.integers(0, 4, L, dtype=np.uint8) for L in QUERY_L]


# ---- lse on arrays ------------------------------------------------------------------------------------------------
def lse_of(*terms):
    """elementwise over the given arrays; all -inf gives -inf"""
    return Lse.arr([np.asarray(t, np.float64) for t in terms])


def lse_all(v):
    """over one array's elements"""
    v = np.asarray(v, np.float64)
    m = float(np.max(v))
    if m == NEG_INF:
        return NEG_INF
    return m + math.log(float(np.sum(np.exp(v - m))))


# ---- the delete chain as the device lays it out --------------------------------------------------------------------
# A lane holds R consecutive nodes.  Its chain, as a function of the value d_in that enters its first node, is the map
# d_out = lse(c, d_in + s): s the sum of the lane's DD, c the chain run from d_in = -inf.  `first` followed by `then`
# is (s1 + s2, lse(c2, c1 + s2)).
def lane_maps(own, dd):
    """own, dd: [64, R] in chain order -> (s, c) per lane"""
    c, s = own[:, 0].copy(), dd[:, 0].copy()
    for r in range(1, own.shape[1]):
        c = lse_of(own[:, r], c + dd[:, r])
        s = s + dd[:, r]
    return s, c


def scan_maps(s, c, skip):
    """inclusive scan in chain order: after the step o, position i holds the composition of positions i - 2 o + 1 .. i;
    a position with fewer than o before it keeps what it has"""
    for o in STEPS:
        if o == skip:
            continue
        s1, c1 = s[:-o], c[:-o]  # the maps of the positions o before
        s2, c2 = s[o:], c[o:]
        c = np.concatenate([c[:o], lse_of(c2, c1 + s2)])
        s = np.concatenate([s[:o], s1 + s2])
    return s, c


def chunk_chain(own, dd, carry, R, skip):
    """one chunk of 64 R nodes in chain order: x_i = lse(own_i, x_{i-1} + dd_i), x_{-1} = carry.  Returns x and, per
    lane, the value that entered its first node."""
    own, dd = own.reshape(64, R), dd.reshape(64, R)
    s, c = scan_maps(*lane_maps(own, dd), skip)
    # the composed map of the lanes before, applied to the carry; the first lane has none before it: the identity (0, -inf)
    sb, cb = np.concatenate([[0.0], s[:-1]]), np.concatenate([[NEG_INF], c[:-1]])
    d_in = lse_of(cb, carry + sb)
    x = np.empty_like(own)
    x[:, 0] = lse_of(own[:, 0], d_in + dd[:, 0])
    for r in range(1, R):
        x[:, r] = lse_of(own[:, r], x[:, r - 1] + dd[:, r])
    return x.reshape(-1), d_in


def padded(t8, em, M):
    """columns padded to whole chunks with -inf, as the kernels take columns at or past core_size"""
    chunk = chunk_of(M)
    ld = -(-M // chunk) * chunk
    t8p, emp = np.full((8, ld), NEG_INF), np.full((em.shape[0], ld), NEG_INF)
    t8p[:, :M], emp[:, :M] = t8, em
    return t8p, emp, chunk, ld


def shifted_up(v, fill=NEG_INF):
    """node k - 1's value at node k"""
    return np.concatenate([[fill], v[:-1]])


def shifted_down(v, fill=NEG_INF):
    """node k + 1's value at node k"""
    return np.concatenate([v[1:], [fill]])


def codes_ending(seq, j):
    """{l: code of x[j - l .. j)}"""
    out = {}
    for l in range(1, min(5, j) + 1):
        v = 0
        for b in seq[j - l:j]:
            v = (v << 2) | int(b)
        out[l] = CODE_OFF[l - 1] + v
    return out


def forward_emulated(t8, em, ei, en, xt, seq, skip=None, cut=()):
    """(null, alt): the Forward recursion with the delete chain per chunk as the device forms it.
    skip: a scan step left out.  cut: chunk carries severed -- "ed" D of the chunk's last node into the next chunk's
    chain, "em" its M into the next chunk's first M -> D candidate, "bm" / "bi" / "bd" its M, I, D into the next chunk's
    first P."""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    M, L = t8.shape[1], len(seq)
    t8, em, chunk, ld = padded(t8, em, M)
    R = chunk // 64
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB = (float(v) for v in xt)
    firsts = np.arange(chunk, ld, chunk)  # the first column of every chunk but the first
    P, Q = np.full((L + 1, ld), NEG_INF), np.full((L + 1, ld), NEG_INF)
    PN, PJ, PC, PR = ([NEG_INF] * (L + 1) for _ in range(4))
    P[0] = (0.0 + SB) + ENT
    PN[0], PR[0] = 0.0 + SN, 0.0
    E, Cc, Rr = NEG_INF, NEG_INF, NEG_INF
    for j in range(1, L + 1):
        code = codes_ending(seq, j)
        Mr = lse_of(*[P[j - l] + em[cd] for l, cd in code.items()])
        Ir = lse_of(*[Q[j - l] + ei[cd] for l, cd in code.items()])
        N, J, Cc, Rr = (Lse.sc([X[j - l] + float(en[cd]) for l, cd in code.items()]) for X in (PN, PJ, PC, PR))
        own = shifted_up(Mr) + MD  # M_{k-1} + MD_k
        if "em" in cut:
            own[firsts] = NEG_INF
        D, carry = np.empty(ld), NEG_INF
        for k0 in range(0, ld, chunk):
            D[k0:k0 + chunk], _ = chunk_chain(own[k0:k0 + chunk], DD[k0:k0 + chunk], carry, R, skip)
            carry = NEG_INF if "ed" in cut else D[k0 + chunk - 1]
        E = lse_all(np.concatenate([Mr, D]))
        B = Lse.sc([N + NB, E + EB, J + JB])
        pm, pi, pd = shifted_up(Mr), shifted_up(Ir), shifted_up(D)
        for name, v in (("bm", pm), ("bi", pi), ("bd", pd)):
            if name in cut:
                v[firsts] = NEG_INF
        P[j] = lse_of(B + ENT, pm + MM, pi + IM, pd + DM)
        Q[j] = lse_of(Mr + MI, Ir + II)
        PN[j], PJ[j], PC[j], PR[j] = N + NN, Lse.sc([E + EJ, J + JJ]), Lse.sc([E + EC, Cc + CC]), Rr + RR
    return Rr, Lse.sc([E + ET, Cc + CT])


def backward_emulated(t8, em, ei, en, xt, seq, skip=None, cut=()):
    """alt_bwd: the Backward recursion with the delete chain running down in k, per chunk in falling
    order, the lanes' order reversed: a node's own part is g_k = lse(bE, DM_{k+1} + bP_{k+1}) (bE in a padded column),
    the step into it DD_{k+1} (-inf in a padded column).  cut: "bD" / "bP" the next chunk's first node's bD / bP into
    the chunk's last node."""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    M, L = t8.shape[1], len(seq)
    t8, em, chunk, ld = padded(t8, em, M)
    R = chunk // 64
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    nMM, nIM, nDM, nMD, nDD = (shifted_down(v) for v in (MM, IM, DM, MD, DD))  # the transitions into node k + 1
    RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB = (float(v) for v in xt)
    lasts = np.arange(chunk - 1, ld - 1, chunk)  # the last column of every chunk but the last
    bM, bI = np.full((L + 6, ld), NEG_INF), np.full((L + 6, ld), NEG_INF)
    bN, bJ, bC = ([NEG_INF] * (L + 6) for _ in range(3))
    bB = bPN = NEG_INF
    for j in range(L, -1, -1):
        code = {l: codes_ending(seq, j + l)[l] for l in range(1, 6) if j + l <= L}  # of x[j .. j + l)
        if code:
            bP = lse_of(*[em[cd] + bM[j + l] for l, cd in code.items()])
            bQ = lse_of(*[ei[cd] + bI[j + l] for l, cd in code.items()])
            bPN, bPJ, bPC = (Lse.sc([float(en[cd]) + X[j + l] for l, cd in code.items()]) for X in (bN, bJ, bC))
        else:
            bP, bQ = np.full(ld, NEG_INF), np.full(ld, NEG_INF)
            bPN = bPJ = bPC = NEG_INF
        bB = lse_all(ENT + bP)
        last = j == L
        bC[j] = Lse.sc([CT if last else NEG_INF, CC + bPC])
        bJ[j] = Lse.sc([JB + bB, JJ + bPJ])
        bN[j] = Lse.sc([NB + bB, NN + bPN])
        bE = Lse.sc([ET if last else NEG_INF, EB + bB, EJ + bPJ, EC + bPC])
        bPn = shifted_down(bP)
        if "bP" in cut:
            bPn[lasts] = NEG_INF
        g = lse_of(np.full(ld, bE), nDM + bPn)
        dn, carry = np.empty(ld), NEG_INF  # dn: bD_{k+1} at node k
        for k0 in range(ld - chunk, -1, -chunk):
            # chain order is falling k: reverse the chunk, lane 63's last node first
            x, d_in = chunk_chain(g[k0:k0 + chunk][::-1], nDD[k0:k0 + chunk][::-1], carry, R, skip)
            d = x[::-1]
            dn[k0:k0 + chunk - 1] = d[1:]
            dn[k0 + chunk - 1] = d_in[0]  # what entered the chunk: the carry itself
            carry = NEG_INF if "bD" in cut else d[0]
        bM[j] = lse_of(np.full(ld, bE), nMD + dn, nMM + bPn, MI + bQ)
        bI[j] = lse_of(nIM + bPn, II + bQ)
    return Lse.sc([SB + bB, SN + bPN])


# ---- tables ---------------------------------------------------------------------------------------------------------
_TABLES = {}


def tables(orc, family, M, L, k=None, eps=EPS):
    """the oracle's f64 tables of the world's profile set up for L, multi-hit, and a random sequence"""
    key = (family, M, L, k, eps)
    if key not in _TABLES:
        p = orc.new(*chain_params(family, M, k), ENTRY_DIST_OCCUPANCY, eps)
        p.setup(L, True, False)
        seq = np.random.default_rng(7).integers(0, 4, L, dtype=np.uint8)
        _TABLES[key] = p.export() + (seq,)
    return _TABLES[key]


def moved(got, base):
    """|delta| / (|x| + 1); both finite"""
    assert math.isfinite(got) and math.isfinite(base), (got, base)
    return abs(got - base) / (abs(base) + 1.0)


def lg(x):
    return "0" if x == 0.0 else "2^%.1f" % math.log2(x)


def knock_outs(tabs, M):
    """{(sweep, what): |delta| / (|x| + 1) of the alt score} for every scan step and, wide profiles, every carry cut"""
    f0, b0 = forward_emulated(*tabs)[1], backward_emulated(*tabs)
    out = {}
    for o in STEPS:
        out["fwd", "o=%d" % o] = moved(forward_emulated(*tabs, skip=o)[1], f0)
        out["bwd", "o=%d" % o] = moved(backward_emulated(*tabs, skip=o), b0)
    if nodes_per_lane(M) == 0:
        for c in FWD_CUTS:
            out["fwd", c] = moved(forward_emulated(*tabs, cut=tuple(c.split("+")))[1], f0)
        for c in BWD_CUTS:
            out["bwd", c] = moved(backward_emulated(*tabs, cut=(c,)), b0)
    return out


def report(title, out):
    for sweep in ("fwd", "bwd"):
        print("%s %s: %s" % (title, sweep, "  ".join("%s %s" % (w, lg(v)) for (s, w), v in out.items() if s == sweep)))


# ---- the world's definition -------------------------------------------------------------------------------------------
def test_the_worlds_are_what_the_docstring_says():
    specs = world_specs()
    assert len(specs) == len(DELETE_M) + len(POSITIVE_M) + len(SEVERED) + len(EPS0_M) == 22
    assert [nodes_per_lane(M) for M in DELETE_M] == [1, 2, 4, 0, 0, 0, 0] and DELETE_M[-1] == 4096
    assert all(M == 64 * nodes_per_lane(M) for M in DELETE_M[:3])  # full classes: lane 63 holds real nodes
    for M, k in SEVERED:
        R = nodes_per_lane(M)
        assert M in DELETE_M and (k in (256, 512) if R == 0 else k in (32 * R, 64 * R - 1)) and 0 < k < M
        null, match, trans = chain_params("severed", M, k)
        whole = chain_params("delete", M)
        cutcols = np.zeros(trans.shape, bool)
        cutcols[k, 2] = cutcols[k, 6] = True
        assert np.isneginf(trans[cutcols]).all() and np.array_equal(trans[~cutcols], whole[2][~cutcols])
        assert np.array_equal(match, whole[1]) and np.array_equal(null, whole[0])
    assert [len(s) for s in world_queries()] == [1, 6, 12, 40]
    import test_forward_pairs
    import test_posterior_pairs
    assert test_forward_pairs.ALLOW == test_posterior_pairs.ALLOW == 2.0 ** -32 == BOUND / 64  # what the GPU file allows
    for M in POSITIVE_M:
        trans = chain_params("positive", M)[2]
        assert (trans[1:M, 2] > 0).all() and (trans[1:M, 6] > 0).all() and trans[1:M, 6].sum() > 25


# ---- premise 0 ------------------------------------------------------------------------------------------------------
CASES0 = ([("delete", M, L, None, EPS) for M, L in PREMISE_SHAPES] + [("positive", M, 12, None, EPS) for M in POSITIVE_M] +
          [("severed", 64, 12, 63, EPS), ("severed", 128, 12, 64, EPS), ("severed", 513, 12, 256, EPS),
           ("delete", 257, 6, None, EPS), ("eps0", 600, 12, None, 0.0), ("pfam", 513, 12, None, EPS)])


@pytest.mark.parametrize("family,M,L,k,eps", CASES0)
def test_premise0_the_emulation_is_the_recursion(dcp, oracle64, family, M, L, k, eps):
    tabs = tables(oracle64, family, M, L, k, eps)
    fn, fa = forward_emulated(*tabs)
    ba = backward_emulated(*tabs)
    pn, pa = forward_plain(*tabs, Lse)
    both = both_plain(*tabs)
    for got, want in ((fn, pn), (fa, pa), (fa, both["alt_fwd"]), (ba, both["alt_bwd"])):
        assert moved(got, want) <= EQUAL, (got, want)
    # the GPU file's reference is the host twin: what moves the emulation by BOUND moves away from the twin as well
    tn, ta = dcp.forward_tables(*tabs)
    twin = dcp.posterior_tables(*tabs)
    for got, want in ((tn, fn), (ta, fa), (twin[3], fa), (twin[4], ba)):
        assert moved(got, want) <= 2.0 ** -32, (got, want)
    print("emulation vs plain %s M %d L %d: fwd %.2e bwd %.2e; alt %.4f" % (family, M, L, moved(fa, pa),
                                                                           moved(ba, both["alt_bwd"]), fa))
    assert moved(ba, fa) <= 2.0 ** -32


def test_premise0_epsilon_zero_is_minus_infinity_in_every_chunk(oracle64):
    for M in EPS0_M:
        for L in (1, 7, 10):  # L mod 3 != 0: no path emits the sequence in codons alone
            tabs = tables(oracle64, "eps0", M, L, None, 0.0)
            assert forward_emulated(*tabs) == (NEG_INF, NEG_INF) and backward_emulated(*tabs) == NEG_INF
            assert forward_plain(*tabs, Lse) == (NEG_INF, NEG_INF)


# ---- premise 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,L", PREMISE_SHAPES)
def test_premise1_every_scan_step_and_carry_moves_the_delete_heavy_score(oracle64, M, L):
    out = knock_outs(tables(oracle64, "delete", M, L), M)
    report("delete-heavy M %d L %d" % (M, L), out)
    assert len(out) == (12 if nodes_per_lane(M) else 12 + len(FWD_CUTS) + len(BWD_CUTS))
    for what, v in out.items():
        # the insert state's carry taken alone needs an insert at a chunk's edge: in 6 rows that weighs 2^-36.9, printed
        # above; it is asserted with bm and bd here, and alone at 12 rows below (the shape changed, not the bound)
        if what == ("fwd", "bi") and L < 12:
            continue
        assert v >= BOUND, (what, lg(v))


@pytest.mark.parametrize("M,L", [(513, 12), (1100, 12)])
def test_premise1_the_insert_carry_alone(oracle64, M, L):
    tabs = tables(oracle64, "delete", M, L)
    v = moved(forward_emulated(*tabs, cut=("bi",))[1], forward_emulated(*tabs)[1])
    print("delete-heavy M %d L %d fwd: bi %s" % (M, L, lg(v)))
    assert v >= BOUND


# ---- premise 2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", POSITIVE_M)
def test_premise2_the_farthest_step_moves_the_positive_chain_score(oracle64, M):
    tabs = tables(oracle64, "positive", M, 12)
    f, b = moved(forward_emulated(*tabs, skip=32)[1], forward_emulated(*tabs)[1]), moved(backward_emulated(*tabs, skip=32),
                                                                                         backward_emulated(*tabs))
    print("positive chain M %d L 12, o = 32 left out: fwd %s bwd %s" % (M, lg(f), lg(b)))
    assert f >= BOUND and b >= BOUND


# ---- premise 3 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k", SEVERED)
def test_premise3_the_cut_lies_where_the_weight_is(oracle64, M, k):
    L = 6 if M == 1100 else 12
    whole, cut = tables(oracle64, "delete", M, L), tables(oracle64, "severed", M, L, k)
    assert np.array_equal(whole[5], cut[5]) and np.array_equal(whole[1], cut[1])
    assert np.isneginf(cut[0][[4, 5], k]).all() and np.isfinite(whole[0][[4, 5], k]).all()  # MD_k, DD_k
    f, b = moved(forward_emulated(*cut)[1], forward_emulated(*whole)[1]), moved(backward_emulated(*cut), backward_emulated(*whole))
    print("severed at %d of %d nodes, L %d: fwd %s bwd %s" % (k, M, L, lg(f), lg(b)))
    assert f > BOUND and b > BOUND


# ---- the gap: the same knock-outs in the pfam-like world, printed ------------------------------------------------------
def test_the_pfam_like_world_cannot_see_the_far_steps(oracle64):
    """Printed, not asserted: in the world of tests/test_forward_pairs.py what the far scan steps bring in lies below
    2^-32 (|x| + 1)."""
    for M, L in PREMISE_SHAPES:
        report("pfam-like M %d L %d" % (M, L), knock_outs(tables(oracle64, "pfam", M, L), M))
