"""Forward scores of a pair list: dcp_forward_tables (the host twin) and dcp_gpu_forward_pairs / Scanner.forward_pairs.

Forward is the scan's recursion with every max replaced by lse(c_1 .. c_n) = mm + log(sum exp(c_i - mm)), mm the
largest term (0 if that is -inf), the terms added in index order.

CPU: a numpy restatement of the recursion takes its combiner as a parameter -- with max it is the oracle's f64
     dp_tables in bits (the structure), with lse it is what the host twin is held against; edge values; refusals;
     tests/c/asan_forward.c under ASan + UBSan as a program of its own.
GPU: per precision the device against the host twin on the tables the device holds, for profiles on every edge of the
     kernel's classes and chunks and queries of 1 .. 333 nt; few wavefronts (hooks build); lists; explicit transitions;
     other batches; the scan untouched; refusals; timing.

The allowance, on both scores: |delta| <= 2^-32 (|x| + 1); -inf compares by equality.  lse is a convex combination in
its arguments, so an absolute error in a candidate reaches the result with weight at most 1 and errors add along the
longest chain of operations behind a value: about 8 (L + M) operations of about 4 ulp each, for L + M <= 1 200 about
2^-38 |x|.  Measured maxima of |delta| / (|x| + 1): see DESIGN section 19."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, np_revcomp, refused
from test_gpu_parity import pfam_like_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
ALLOW = 2.0 ** -32
CODE_OFF = (0, 4, 20, 84, 340)
SHAPES = ((2, 1), (2, 7), (5, 30), (64, 100), (65, 60), (40, 333))  # (M, L)
PRECISIONS = (32, 64)
FLAGS = ((True, False), (False, False), (True, True))  # (multi_hits, hmmer3_compat)


def within(got, want):
    """the allowance; -inf by equality; never NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]) or np.isinf(got[~inf]).any():
        return False
    return bool(np.all(np.abs(got[~inf] - want[~inf]) <= ALLOW * (np.abs(want[~inf]) + 1.0)))


def worst(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) + 1.0))) if fin.any() else 0.0


# ---- the restatement: one recursion, the combiner a parameter -----------------------------------------------------
class Max:
    @staticmethod
    def arr(c):
        return np.max(np.stack(c), axis=0)

    sc = staticmethod(max)


class Lse:
    @staticmethod
    def arr(c):
        c = np.stack(c)
        m = np.max(c, axis=0)
        mm = np.where(np.isneginf(m), 0.0, m)
        s = np.zeros_like(mm)
        for row in c:  # index order
            s = s + np.exp(row - mm)
        with np.errstate(divide="ignore"):
            return mm + np.log(s)

    @staticmethod
    def sc(c):
        m = max(c)
        mm = 0.0 if m == NEG_INF else m
        s = 0.0
        for v in c:
            s += math.exp(v - mm)
        return mm + math.log(s) if s > 0.0 else NEG_INF


def restate(t8, em, ei, en, xt, seq, comb):
    """(null, alt): dp_tables_run of oracle/oracle.c in double with `comb` where it has max"""
    t8, em, ei, en, xt = (np.asarray(a, np.float64) for a in (t8, em, ei, en, xt))
    ENT, MM, IM, DM, MD, DD, MI, II = t8
    RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB = (float(v) for v in xt)
    M, L = t8.shape[1], len(seq)
    P, Q = np.full((L + 1, M), NEG_INF), np.full((L + 1, M), NEG_INF)
    PN, PJ, PC, PR = ([NEG_INF] * (L + 1) for _ in range(4))
    P[0] = (0.0 + SB) + ENT
    PN[0], PR[0] = 0.0 + SN, 0.0
    w, E, Cc, Rr = 0, NEG_INF, NEG_INF, NEG_INF
    for j in range(1, L + 1):
        w = ((w << 2) | int(seq[j - 1])) & 1023
        ls = range(1, min(5, j) + 1)
        code = {l: CODE_OFF[l - 1] + (w & ((1 << (2 * l)) - 1)) for l in ls}
        Mr = comb.arr([P[j - l] + em[code[l]] for l in ls])
        Ir = comb.arr([Q[j - l] + ei[code[l]] for l in ls])
        N = comb.sc([PN[j - l] + float(en[code[l]]) for l in ls])
        J = comb.sc([PJ[j - l] + float(en[code[l]]) for l in ls])
        Cc = comb.sc([PC[j - l] + float(en[code[l]]) for l in ls])
        Rr = comb.sc([PR[j - l] + float(en[code[l]]) for l in ls])
        D = [NEG_INF] * M
        a, dd = (Mr[:-1] + MD[1:]).tolist(), DD.tolist()
        for k in range(1, M):
            D[k] = comb.sc([a[k - 1], D[k - 1] + dd[k]])
        terms, mr = [], Mr.tolist()
        for k in range(M):
            terms.append(mr[k])
            if k:
                terms.append(D[k])
        E = comb.sc(terms)
        B = comb.sc([N + NB, E + EB, J + JB])
        D = np.array(D)
        P[j, 0] = B + ENT[0]
        if M > 1:
            P[j, 1:] = comb.arr([B + ENT[1:], Mr[:-1] + MM[1:], Ir[:-1] + IM[1:], D[:-1] + DM[1:]])
        Q[j] = comb.arr([Mr + MI, Ir + II])
        PN[j], PJ[j], PC[j], PR[j] = N + NN, comb.sc([E + EJ, J + JJ]), comb.sc([E + EC, Cc + CC]), Rr + RR
    return Rr, comb.sc([E + ET, Cc + CT])


_CASES = {}


def oracle_case(orc, M, L, multi, eps=0.01):
    """the oracle's exported tables of sample(100 + M, M) set up for L, and a random sequence"""
    key = (orc.np, M, L, multi, eps)
    if key not in _CASES:
        p = orc.sample(100 + M, M, ENTRY_DIST_OCCUPANCY, eps)
        p.setup(L, multi, False)
        seq = np.random.default_rng(1000 * M + L).integers(0, 4, L, dtype=np.uint8)
        _CASES[key] = p.export() + (seq,)
    return _CASES[key]


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_structure_with_max_is_the_oracle(oracle64, M, L, multi):
    t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, multi)
    rc, on, oa = oracle64.dp_tables(t8, em, ei, en, xt, bytes(seq))
    assert rc == 0
    gn, ga = restate(t8, em, ei, en, xt, seq, Max)
    assert bits(np.array([gn, ga])).tolist() == bits(np.array([on, oa])).tolist()


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("M,L", SHAPES)
def test_host_twin_against_the_restatement(dcp, oracle64, oracle32, M, L, multi):
    for orc in (oracle64, oracle32):  # float tables go in as they are: promoted to double
        t8, em, ei, en, xt, seq = oracle_case(orc, M, L, multi)
        want = restate(t8, em, ei, en, xt, seq, Lse)
        got = dcp.forward_tables(t8, em, ei, en, xt, seq)
        print("host twin vs restatement M %d L %d multi %d f%d: %.3e" % (M, L, multi, 64 if orc is oracle64 else 32,
                                                                         worst(got, want)))
        assert within(got, want), (got, want)
        assert np.isfinite(got).all()
        rc, vn, va = orc.dp_tables(t8, em, ei, en, xt, bytes(seq))
        assert rc == 0
        if orc is oracle64:  # all paths weigh at least as much as the best one (the float oracle rounds its sums to float)
            assert got[0] >= vn - ALLOW * (abs(vn) + 1) and got[1] >= va - ALLOW * (abs(va) + 1)
        if L == 1:  # one word, one path through R
            assert bits(np.array([got[0]])) == bits(np.array([float(vn)]))


def test_epsilon_zero_is_minus_infinity_not_nan(dcp, oracle64):
    for L in (1, 7, 10):  # L mod 3 != 0: no path emits the sequence in codons alone
        t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, L, True, eps=0.0)
        assert dcp.forward_tables(t8, em, ei, en, xt, seq) == (NEG_INF, NEG_INF)
    t8, em, ei, en, xt, seq = oracle_case(oracle64, 5, 9, True, eps=0.0)
    assert np.isfinite(dcp.forward_tables(t8, em, ei, en, xt, seq)).all()


def test_padding_columns_change_no_bit(dcp, oracle64):
    for M, L in ((2, 7), (5, 30), (65, 60)):
        t8, em, ei, en, xt, seq = oracle_case(oracle64, M, L, True)
        ldk = M + 7
        t8p, emp = np.full((8, ldk), NEG_INF), np.full((1364, ldk), NEG_INF)
        t8p[:, :M], emp[:, :M] = t8, em
        null, alt = C.c_double(1.0), C.c_double(2.0)
        rc = dcp.lib.dcp_forward_tables(M, ldk, t8p.ctypes.data, emp.ctypes.data, ei.ctypes.data, en.ctypes.data,
                                        xt.ctypes.data, seq.ctypes.data, L, C.byref(null), C.byref(alt))
        assert rc == 0
        want = dcp.forward_tables(t8, em, ei, en, xt, seq)
        assert bits(np.array([null.value, alt.value])).tolist() == bits(np.array(want)).tolist()
        # and all of them as columns of the profile: -inf transitions keep them out of every sum
        assert bits(np.array(dcp.forward_tables(t8p, emp, ei, en, xt, seq))).tolist() == bits(np.array(want)).tolist()


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
        null, alt = C.c_double(1.5), C.c_double(2.5)
        rc = dcp.lib.dcp_forward_tables(a["M"], a["ldk"], a["t8"], a["em"], a["ei"], a["en"], a["xt"], a["seq"], a["L"],
                                        C.byref(null), C.byref(alt))
        assert rc == dcp.RC_EINVAL and (null.value, alt.value) == (1.5, 2.5), change
    null = C.c_double(1.5)
    for outs in ((None, C.byref(null)), (C.byref(null), None)):
        assert dcp.lib.dcp_forward_tables(5, 5, P(t8), P(em), P(ei), P(en), P(xt), P(seq), 30, *outs) == dcp.RC_EINVAL
        assert null.value == 1.5
    with pytest.raises(dcp.DcpError):
        dcp.forward_tables(t8, em[:, :4], ei, en, xt, seq)


def test_forward_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_forward.c with the host model alone (no device code) under ASan + UBSan, as a program of its
    own."""
    obj, exe = str(tmp_path / "asan_forward.o"), str(tmp_path / "asan_forward")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_forward.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_forward ok" in r.stdout


# ---- GPU: the device against the host twin -----------------------------------------------------------------------
WORLD_M = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1100)  # and a flagged profile of 90 nodes behind them
WORLD_L = (1, 2, 4, 5, 6, 16, 17, 100, 333)
_WORLD = {}


def device_tables(dcp, sc, profs, precision, eps):
    """per profile (trans8, match, insert, null) as the device holds them"""
    out = []
    for p, prof in enumerate(profs):
        if precision == 64:
            out.append((prof.parts64()[0], sc.match_table(p)) + sc.insert_null_tables64(p))
        else:
            out.append((prof.trans8, sc.match_table(p), dcp.frame_table_host(prof.insert_dist, eps),
                        dcp.frame_table_host(prof.null_dist, eps)))
    return out


def xtrans_of(dcp, precision, L, multi, h3):
    return (dcp.xtrans64 if precision == 64 else dcp.xtrans)(L, multi, h3)


def twin(dcp, tabs, xt, seq):
    return dcp.forward_tables(*tabs, xt, seq)


def world(dcp, precision, orc64):
    """profiles, queries, the device's tables, and per flags: the host twin's scores, the dense row-sweep scan's, and
    the Viterbi scores in double on the same tables (the oracle's f64 dp_tables: on a double DB the dense scan's bits;
    a float DB's dense scan rounds every sum to float, so its score may exceed the weight of its own best path)"""
    if precision not in _WORLD:
        rng = np.random.default_rng(1900 + precision)
        params = [pfam_like_params(rng, M) for M in WORLD_M]
        null, match, trans = pfam_like_params(rng, 90)
        trans = trans.copy()
        trans[1:90, 2] = np.float32(0.7)  # MD > 0 (and DD): the construction of tests/test_scan_pairs.py
        trans[1:90, 6] = np.float32(0.4)
        params.append((null, match, trans))
        eps = float(np.float32(0.01))
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, eps)
        profs = [dcp.ProteinProfile.from_params(*prm, cfg, f"FWD{i}", precision=precision) for i, prm in enumerate(params)]
        seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in WORLD_L]
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        tabs = device_tables(dcp, sc, profs, precision, eps)
        ref, dense, vit = {}, {}, {}
        for multi, h3 in FLAGS:
            sc.scan(multi, h3, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
            dense[multi, h3] = tuple(np.asarray(a, np.float64) for a in sc.scores())
            fn, fa = np.zeros((len(seqs), len(profs))), np.zeros((len(seqs), len(profs)))
            vn, va = np.zeros_like(fn), np.zeros_like(fa)
            for q, s in enumerate(seqs):
                assert np.array_equal(sc.fetch_seq(q), s)
                xt = xtrans_of(dcp, precision, len(s), multi, h3)
                for p in range(len(profs)):
                    fn[q, p], fa[q, p] = twin(dcp, tabs[p], xt, s)
                    rc, vn[q, p], va[q, p] = orc64.dp_tables(*tabs[p], xt, bytes(s))
                    assert rc == 0
            ref[multi, h3], vit[multi, h3] = (fn, fa), (vn, va)
        sc.close()
        _WORLD[precision] = (profs, seqs, tabs, ref, dense, vit)
    return _WORLD[precision]


def loaded(dcp, precision, lib=None):
    profs, seqs = _WORLD[precision][:2]
    sc = dcp.Scanner(0, lib=lib) if lib else dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pair_against_the_host_twin(dcp, oracle64, precision, multi, h3):
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    every = [(q, p) for q in range(len(seqs)) for p in range(len(profs))]
    order = np.random.default_rng(11).permutation(len(every))
    sq, pr = np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])
    sc = loaded(dcp, precision)
    gn, ga = sc.forward_pairs(sq, pr, multi, h3)
    sc.close()
    fn, fa = ref[multi, h3][0][sq, pr], ref[multi, h3][1][sq, pr]
    print("device vs host twin f%d multi %d h3 %d: null %.3e alt %.3e" % (precision, multi, h3, worst(gn, fn), worst(ga, fa)))
    assert within(gn, fn) and within(ga, fa)
    # finite exactly where the dense row-sweep scan's scores are
    dn, da = dense[multi, h3][0][sq, pr], dense[multi, h3][1][sq, pr]
    assert np.array_equal(np.isfinite(gn), np.isfinite(dn)) and np.array_equal(np.isfinite(ga), np.isfinite(da))
    assert np.isfinite(ga).sum() > len(every) // 2
    # and at least the best path's weight there: the Viterbi score in double on the same tables
    vn, va = vit[multi, h3][0][sq, pr], vit[multi, h3][1][sq, pr]
    if precision == 64:
        assert np.array_equal(bits(vn), bits(dn)) and np.array_equal(bits(va), bits(da))
    for name, g, v, d in (("null", gn, vn, dn), ("alt", ga, va, da)):
        fin = np.isfinite(v)
        assert np.array_equal(fin, np.isfinite(d))
        print("  %s: largest (Viterbi - Forward) / (|Viterbi| + 1): in double %.3e, the dense scan's %.3e" % (
            name, np.max((v[fin] - g[fin]) / (np.abs(v[fin]) + 1.0)), np.max((d[fin] - g[fin]) / (np.abs(d[fin]) + 1.0))))
        assert np.all(g[fin] >= v[fin] - ALLOW * (np.abs(v[fin]) + 1.0))
    # summing paths matters: somewhere Forward lies clearly above Viterbi
    assert np.max(ga[np.isfinite(va)] - va[np.isfinite(va)]) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_few_wavefronts_change_no_bit(dcp, oracle64, precision):
    """the stride loop's second trip, a grid that is not a multiple of four wavefronts, a wide pair behind a narrower
    one in the same work area"""
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    ix = {M: i for i, M in enumerate(WORLD_M)}
    q = WORLD_L.index(100)
    pairs = [(q, ix[1100]), (q, ix[257]), (q, ix[1100]), (q, ix[2]), (q, ix[513])]
    pairs += [(8, ix[512]), (7, ix[64]), (8, ix[129]), (5, ix[1100]), (8, len(WORLD_M)), (6, ix[256])]
    sq, pr = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    sc = loaded(dcp, precision, dcp.load_testhooks())
    base = sc.forward_pairs(sq, pr)
    assert within(base[0], ref[True, False][0][sq, pr]) and within(base[1], ref[True, False][1][sq, pr])
    for cap in (3, 1, 0):
        sc.test_set_forward_waves(cap)
        got = sc.forward_pairs(sq, pr)
        assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1])), cap
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lists_come_back_in_list_order(dcp, oracle64, precision):
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    fn, fa = ref[True, False]
    sc = loaded(dcp, precision)
    assert sc.forward_kernel_ms < 0  # none has run
    gn, ga = sc.forward_pairs([], [])
    assert gn.shape == (0,) and ga.shape == (0,) and gn.dtype == np.float64 and sc.forward_kernel_ms < 0
    gn, ga = sc.forward_pairs([8], [9])
    assert within(gn, fn[8:9, 9]) and within(ga, fa[8:9, 9])
    assert sc.forward_kernel_ms > 0
    sq, pr = np.array([7, 8, 7, 7, 3, 8]), np.array([11, 4, 11, 11, 0, 4])
    gn, ga = sc.forward_pairs(sq, pr)
    assert within(gn, fn[sq, pr]) and within(ga, fa[sq, pr])
    assert len({int(b) for b in bits(ga)[[0, 2, 3]]}) == 1 and bits(ga)[1] == bits(ga)[5]  # a pair listed twice is scored twice
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_transitions_in_the_dbs_precision(dcp, oracle64, precision):
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    # every sequence with the uni-hit transitions of a sequence of 50 more bases: nothing the flags could derive
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    sq, pr = np.array([8, 7, 4, 8, 2]), np.array([12, 9, 5, 11, 1])
    gn, ga = sc.forward_pairs(sq, pr, True, False)  # the flags are ignored
    want = np.array([twin(dcp, tabs[p], xt[q], seqs[q]) for q, p in zip(sq, pr)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    assert not within(ga, ref[True, False][1][sq, pr])
    # those of the other precision are refused, as a scan refuses them
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.forward_pairs(sq, pr))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_batches(dcp, oracle64, precision):
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    eps0 = dcp.ProteinProfile.sample(77, 70, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    mine = [profs[3], eps0, profs[8], profs[12]]
    sc = dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs(seqs)
    mytabs = device_tables(dcp, sc, mine, precision, 0.0)[1:2]
    # an epsilon-0 profile among normal ones: -inf twice where L mod 3 != 0 (elsewhere a stop codon in frame does the
    # same: whatever the host twin says)
    sq = np.arange(len(seqs)).repeat(4)
    pr = np.tile(np.arange(4), len(seqs))
    gn, ga = sc.forward_pairs(sq, pr)
    assert not np.isnan(gn).any() and not np.isnan(ga).any()
    for q, s in enumerate(seqs):
        want = twin(dcp, mytabs[0], xtrans_of(dcp, precision, len(s), True, False), s)
        assert within([gn[4 * q + 1]], [want[0]]) and within([ga[4 * q + 1]], [want[1]])
        if len(s) % 3:
            assert gn[4 * q + 1] == NEG_INF and ga[4 * q + 1] == NEG_INF
    for j, p in ((0, 3), (2, 8), (3, 12)):
        assert within(gn[j::4], ref[True, False][0][:, p]) and within(ga[j::4], ref[True, False][1][:, p])
    sc.close()

    # both strands: resident n + q is the reverse complement of q
    sc = loaded(dcp, precision)
    n = len(seqs)
    sc.add_reverse_strand()
    sq, pr = np.array([n + 8, n + 7, 8, n + 5]), np.array([9, 12, 9, 2])
    gn, ga = sc.forward_pairs(sq, pr)
    want = np.array([twin(dcp, tabs[p], xtrans_of(dcp, precision, len(seqs[q % n]), True, False),
                          np_revcomp(seqs[q % n]) if q >= n else seqs[q % n]) for q, p in zip(sq, pr)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    sc.close()

    # regions cut out of the batch
    sc = loaded(dcp, precision)
    sc.cut_regions([8, 8, 7], [0, 100, 30], [333, 150, 64], [0, 1, 0])
    sq, pr = np.array([0, 1, 2, 1]), np.array([10, 6, 12, 0])
    gn, ga = sc.forward_pairs(sq, pr)
    cut = [seqs[8], np_revcomp(seqs[8][100:250]), seqs[7][30:94]]
    for r, s in enumerate(cut):
        assert np.array_equal(sc.fetch_seq(r), s)
    want = np.array([twin(dcp, tabs[p], xtrans_of(dcp, precision, len(cut[q]), True, False), cut[q]) for q, p in zip(sq, pr)])
    assert within(gn, want[:, 0]) and within(ga, want[:, 1])
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_scan_is_untouched(dcp, oracle64, precision):
    profs, seqs, tabs, ref, dense, vit = world(dcp, precision, oracle64)
    sc = loaded(dcp, precision)
    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    nl, al = sc.scores()
    hits, cells, launches = sc.hits().copy(), sc.cells, sc.last_scan_launches
    assert len(hits) > 0
    sq, pr = np.array([8, 7, 6, 8]), np.array([11, 3, 0, 12])
    gn, ga = sc.forward_pairs(sq, pr, False, False)  # other flags than the scan's
    assert within(ga, ref[False, False][1][sq, pr])
    n2, a2 = sc.scores()
    assert np.array_equal(bits(n2), bits(nl)) and np.array_equal(bits(a2), bits(al))
    assert sc.hits().tobytes() == hits.tobytes() and sc.cells == cells and sc.last_scan_launches == launches
    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    n3, a3 = sc.scores()
    assert np.array_equal(bits(n3), bits(nl)) and np.array_equal(bits(a3), bits(al))
    assert sc.hits().tobytes() == hits.tobytes()
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_outputs(dcp, oracle64, precision):
    profs, seqs = world(dcp, precision, oracle64)[:2]
    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.forward_pairs([0], [0]))  # no DB
    sc.upload_db(profs)
    refused(dcp, sc, lambda: sc.forward_pairs([0], [0]))  # no batch
    sc.upload_seqs(seqs)
    with pytest.raises(dcp.DcpError) as e:
        sc.forward_pairs([0, len(seqs), 99], [0, 0, 99])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    with pytest.raises(dcp.DcpError) as e:
        sc.forward_pairs([0, 1], [0, len(profs)])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    refused(dcp, sc, lambda: sc.forward_pairs([0, 1], [0]))
    sq, pr = np.array([0, 99], np.uint32), np.array([0, 0], np.uint32)
    null, alt = np.full(2, 1.5), np.full(2, 2.5)
    call = sc._lib.dcp_gpu_forward_pairs
    assert call(sc._c, 1, 0, sq.ctypes.data, pr.ctypes.data, 2, null.ctypes.data, alt.ctypes.data) == dcp.RC_EINVAL
    sq[1] = 1
    for args in ((None, pr.ctypes.data, null.ctypes.data, alt.ctypes.data), (sq.ctypes.data, None, null.ctypes.data, alt.ctypes.data),
                 (sq.ctypes.data, pr.ctypes.data, None, alt.ctypes.data), (sq.ctypes.data, pr.ctypes.data, null.ctypes.data, None)):
        assert call(sc._c, 1, 0, args[0], args[1], 2, args[2], args[3]) == dcp.RC_EINVAL
        assert len(sc._lib.dcp_gpu_last_error(sc._c)) > 0
    assert null.tolist() == [1.5, 1.5] and alt.tolist() == [2.5, 2.5]
    assert call(sc._c, 1, 0, None, None, 0, None, None) == 0  # an empty list needs no arrays
    assert sc.forward_kernel_ms < 0
    assert call(sc._c, 1, 0, sq.ctypes.data, pr.ctypes.data, 2, null.ctypes.data, alt.ctypes.data) == 0
    assert sc.forward_kernel_ms > 0 and np.isfinite(null).all() and null[0] != 1.5
    sc.close()
