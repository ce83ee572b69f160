"""The cases of tests/test_pair_mode_edges.py and what they rest on, checked on the CPU.

Pair mode -- viterbi_rowsweep_kernel<R, W, 0, false> with a.pairs set, viterbi64_kernel<R, false, true> -- scores a
list of {query, profile}.  The drivers (dcp_gpu.hip) size its launches:

  float   dcp_gpu_scan_pairs, launch_qlane_scan: min(ceil(n / tpb), 8 x CUs) blocks rounded up to a multiple of 8,
          tpb = dcp_rowsweep_tasks_per_block(W) = 4 for W == 1, else 1; launch_segsweep_class (W > 1): min(n, 8 x CUs)
          rounded up the same way
  double  scan_pairs64: min(n, 2^24) wavefronts, the segmented group (more than 256 nodes) seg_waves = min(n, 2^27 /
          (5 (lmax + 1))) (f64_seg_columns); kernel 4's redo launches: min(seg_waves | 4096, capacity, 4096) -- both
          from f64_group_geometry, the latter with its cap of 4 096

so a block (wavefront) takes a second task only from T + 1 listed pairs on, T = tpb x 8 x CUs (float), seg_waves or
4 096 (double).  Restated here as functions of the CU count, W and lmax, with the list builder of the GPU cases and
the premises that need no device:

  * the builder's lists have the asked length and put, `stride` tasks apart (one block's consecutive tasks), the
    longest query before the 1-nt one, the 1-nt one before the longest, and two profiles of one class back to back;
  * every pair the large lists can name has finite oracle scores, so "every listed pair is a hit at -inf" rests on the
    reference alone (oracle fed the host's expansion of the tables);
  * the flagged profiles' delete states decide E(j): on the oracle's best path E is entered from a delete state;
  * with E -> B and J -> B free and N -> B closed, E(j) is finite in some row of every pair (alt is finite and B can
    only have been entered at row 0): B(j) = E(j) + EB beats N(j) + NB = -inf there, the f64 query-lane kernel's redo
    criterion.
"""
import numpy as np
import pytest

import test_gpu_parity as tp
import test_rowsweep_edge_premises as pr
from oracle_py import B_STATE, E_STATE, ENTRY_DIST_OCCUPANCY

CU_COUNTS = (256, 304, 128, 64)  # the restated rules are checked for these; the GPU cases read the device's
CLASSES = [(r, 1) for r in range(1, 9)] + [(3, 4), (4, 4), (3, 8), (4, 8), (3, 16), (4, 16)]  # kClasses
F64_GROUP_CAPS = (64, 128, 256, 4096)
F64_REDO_WAVES = 4096


# ---- the grid rules, restated --------------------------------------------------------------------------------------
def tpb_of(W):
    """dcp_rowsweep_tasks_per_block"""
    return 4 if W == 1 else 1


def round8(g):
    return (g + 7) // 8 * 8


def float_blocks(n, W, cus):
    """dcp_gpu_scan_pairs / launch_qlane_scan: blocks of a pair launch over a list of n (capacity n)"""
    return round8(min(-(-n // tpb_of(W)), 8 * cus))


def seg_redo_blocks(n, cus):
    """launch_segsweep_class: blocks of the exact kernel over seg_redo (capacity n, W > 1)"""
    return round8(min(n, 8 * cus))


def T_of(W, cus):
    """the longest list no block of which takes a second task"""
    return tpb_of(W) * 8 * cus


def trips(n, units, tpb=1):
    """the most tasks one block (float) / wavefront (double) takes of a list of n"""
    return -(-n // (units * tpb))


def seg_waves(lmax, npairs):
    """f64_seg_columns"""
    return min(npairs, max(1, (1 << 27) // (5 * (lmax + 1)))) if npairs else 0


def f64_pair_waves(g, n, lmax):
    """scan_pairs64: wavefronts over the list of group g"""
    return seg_waves(lmax, n) if g == 3 else min(n, 1 << 24)


def f64_redo_waves(g, cap, nq, nprof3, lmax):
    """scan64, kernel 4: wavefronts over the redo list of group g (capacity cap); the segmented group's columns are
    sized for all its nprof3 x nq pairs"""
    return min(seg_waves(lmax, nprof3 * nq) if g == 3 else F64_REDO_WAVES, min(cap, F64_REDO_WAVES))


def f64_group_of(M):
    return next(g for g, cap in enumerate(F64_GROUP_CAPS) if M <= cap)


def test_grid_rules():
    for cus in CU_COUNTS:
        G = 8 * cus
        for W in (1, 4, 8, 16):
            tpb, T = tpb_of(W), T_of(W, cus)
            assert T == tpb * G
            for n, want in ((1, 1), (9, 1), (T - 1, 1), (T, 1), (T + 1, 2), (2 * T, 2), (2 * T + 3, 3)):
                b = float_blocks(n, W, cus)
                assert b % 8 == 0 and 8 <= b <= G and trips(n, b, tpb) == want, (cus, W, n, b)
            assert float_blocks(T, W, cus) == G == float_blocks(2 * T + 3, W, cus)
        assert seg_redo_blocks(G, cus) == G == seg_redo_blocks(G + 1, cus) and trips(G + 1, G) == 2
        assert seg_redo_blocks(G - 9, cus) == G - 8
    # the issue's figures for a 256-CU chip
    assert (T_of(1, 256) + 1, T_of(4, 256) + 1, F64_REDO_WAVES + 1) == (8193, 2049, 4097)
    # the segmented group: a second pair per wavefront from seg_waves + 1 listed pairs on
    sw = seg_waves(A64_LMAX, 10 ** 6)
    assert sw == (1 << 27) // (5 * (A64_LMAX + 1)) and 850 <= sw <= 950
    for n, want in ((sw - 1, 1), (sw, 1), (sw + 1, 2), (2 * sw + 3, 3)):
        assert trips(n, f64_pair_waves(3, n, A64_LMAX)) == want
    assert f64_pair_waves(3, sw - 1, A64_LMAX) == sw - 1 and f64_pair_waves(0, 9, 33) == 9
    assert seg_waves(40, 3 * 1366) == 3 * 1366 and f64_redo_waves(3, 3 * 1366, 1366, 3, 40) == 4096
    assert f64_redo_waves(3, 1, 1366, 3, 40) == 1 and f64_redo_waves(0, 4097, 1366, 3, 40) == 4096


# ---- the list builder ----------------------------------------------------------------------------------------------
def build_list(profs, short_q, long_q, one_q, n, stride, wide_q=()):
    """A list of n (query, profile) pairs of ONE class.  profs: the class's profile indices (one or two); short_q: the
    queries of 1 .. 33 nt (one_q, the 1-nt query, among them); long_q: the longest query; wide_q: queries only the
    small lists use.  Deterministic: position i holds combination i of the cycle over short_q x profs (small lists, n
    <= 9: over all queries); then, `stride` = blocks x tasks per block apart -- the consecutive tasks of one block or
    wavefront --
      positions 0, stride, 2 stride:          (long, first profile), (1 nt, last profile), (long, first profile)
      positions 1, 1 + stride, 1 + 2 stride:  a short query against the first, the last, the first profile
    as far as they lie inside the list (position 0 always does: every list names the longest query)."""
    qs = list(short_q) + ([long_q] + list(wide_q) if n <= 9 else [])
    combos = [(q, p) for q in qs for p in profs]
    out = [combos[(i * 5 + i // len(combos)) % len(combos)] for i in range(n)]  # a stride of 5 through the cycle
    mid = short_q[len(short_q) // 2]
    for j, pair in enumerate([(long_q, profs[0]), (one_q, profs[-1]), (long_q, profs[0])]):
        if j * stride < n:
            out[j * stride] = pair
    for j, pair in enumerate([(mid, profs[0]), (mid, profs[-1]), (mid, profs[0])]):
        if 1 + j * stride < n and n > 1:
            out[1 + j * stride] = pair
    return out


def shared_block_neighbours(lst, stride):
    """[(pair, the pair the same block or wavefront takes next)]"""
    return [(lst[i], lst[i + stride]) for i in range(len(lst) - stride)]


def test_list_builder():
    short, long_q, one = [0, 1, 2, 3, 4, 5, 6], 8, 0
    for cus in CU_COUNTS:
        for W, profs in ((1, [3]), (1, [3, 9]), (4, [5, 6]), (16, [7])):
            T = T_of(W, cus)
            for n in (1, 2, 3, 4, 5, 7, 8, 9, T - 1, T, T + 1, 2 * T + 3):
                stride = float_blocks(n, W, cus) * tpb_of(W)
                lst = build_list(profs, short, long_q, one, n, stride, wide_q=[7])
                assert len(lst) == n and lst == build_list(profs, short, long_q, one, n, stride, wide_q=[7])
                assert lst[0] == (long_q, profs[0]) and {p for _, p in lst} <= set(profs)
                nb = shared_block_neighbours(lst, stride)
                assert len(nb) == max(0, n - stride)
                if n <= T:
                    assert not nb
                    continue
                assert ((long_q, profs[0]), (one, profs[-1])) in nb  # the longest query directly before the 1-nt one
                if n == 2 * T + 3:
                    assert ((one, profs[-1]), (long_q, profs[0])) in nb  # and behind it
                    if len(profs) > 1:  # two profiles of one class back to back, the same query
                        assert any(a[0] == b[0] and a[1] != b[1] for a, b in nb)
                    assert 2 <= sum(q == long_q for q, _ in lst) <= 4  # the longest query a few times
                    assert len(set(lst)) >= len(short) * len(profs)  # every short combination occurs
                if n > 9:
                    assert 7 not in {q for q, _ in lst}


# ---- float, case A: scan_pairs over every size class ---------------------------------------------------------------
A_CAPS = [64 * R * W for R, W in CLASSES]
A_SPEC = A_CAPS + [5, 450, 600, 2500, -90]  # a second, smaller profile in (1,1), (8,1), (3,4), (3,16); one flagged
A_LENGTHS = [1, 2, 3, 15, 16, 17, 33, 64, 257]
A_SHORT, A_WIDE, A_LONG, A_ONE = [0, 1, 2, 3, 4, 5, 6], [7], 8, 0  # indices into A_LENGTHS
A_N = ["1", "2", "3", "4", "5", "7", "8", "9", "T-1", "T", "T+1", "2T+3"]
A_MODES = [(True, False), (False, False), (True, True)]  # multi-hit throughout; uni-hit and HMMER3-compatible at T + 1
_a = {}


def a_n(name, T):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}.get(name) or int(name)


def a_case(dcp):
    if "v" not in _a:
        rng = np.random.default_rng(14001)
        profiles = pr.make_profiles(dcp, pr.make_params(rng, A_SPEC), A_SPEC)
        _a["v"] = (profiles, pr.rand_of(rng, A_LENGTHS))
    return _a["v"]


def a_classes():
    """{(R, W): [profile indices]} of A_SPEC"""
    out = {}
    for p, m in enumerate(A_SPEC):
        out.setdefault(pr.class_of(abs(m)), []).append(p)
    return out


def a_lists(name, cus):
    """{(R, W): list} of one scan_pairs call of case A, and the call's list: the classes' lists interleaved, so that
    the driver's bucketing by class has work to do"""
    per = {}
    for (R, W), profs in a_classes().items():
        n = a_n(name, T_of(W, cus))
        per[(R, W)] = build_list(profs, A_SHORT, A_LONG, A_ONE, n, float_blocks(n, W, cus) * tpb_of(W), A_WIDE)
    longest = max(len(v) for v in per.values())
    whole = [v[i] for i in range(longest) for v in per.values() if i < len(v)]
    return per, whole


def test_a_db_and_lists():
    cl = a_classes()
    assert sorted(cl) == sorted(CLASSES) and all(abs(A_SPEC[v[0]]) == 64 * k[0] * k[1] for k, v in cl.items())
    assert {k for k, v in cl.items() if len(v) == 2} == {(1, 1), (2, 1), (8, 1), (3, 4), (3, 16)}
    assert [A_LENGTHS[q] for q in A_SHORT] == [1, 2, 3, 15, 16, 17, 33] and A_LENGTHS[A_LONG] == 257 == max(A_LENGTHS)
    for name in A_N:
        per, whole = a_lists(name, 256)
        assert sorted(whole) == sorted(p for v in per.values() for p in v)
        for (R, W), lst in per.items():
            assert len(lst) == a_n(name, T_of(W, 256)) and {p for _, p in lst} <= set(cl[(R, W)])


def test_a_every_pair_is_finite(dcp, oracle32):
    """All 19 x 9 pairs, in the three modes: finite null and alt, a finite LRT; some pass threshold 10, most do not."""
    profiles, seqs = a_case(dcp)
    tables = [pr.host_table(dcp, p) for p in profiles]
    for mode in A_MODES:
        on, oa = pr.oracle_scores(dcp, oracle32, profiles, tables, seqs, pr.mode_xtrans(dcp, seqs, mode))
        lrt = np.float32(-2) * (on - oa)
        assert np.isfinite(on).all() and np.isfinite(oa).all() and np.isfinite(lrt).all(), mode


# ---- float, cases B and D: the query-lane kernels' redo lists ------------------------------------------------------
B_SPEC = [-m for m in (3, 8, 9, 17, 31, 40, 50, 63, 64, 449, 460, 470, 480, 490, 500, 510, 511, 512, 513, 640, 768)]
B_DISTINCT = 120  # distinct queries: three of every length 1 .. 40
B_W3_SIZES = (3, 4, 5, 6, 7, 8)


def b_classes():
    out = {}
    for p, m in enumerate(B_SPEC):
        out.setdefault(pr.class_of(abs(m)), []).append(p)
    return out


def b_nq(cus):
    """the fewest queries that take every class of B_SPEC past its T"""
    return max(T_of(W, cus) // len(v) + 1 for (_, W), v in b_classes().items())


def b_queries(rng, nq):
    """nq queries of 1 .. 40 nt, copies of B_DISTINCT distinct ones in a random order"""
    base = pr.rand_of(rng, [1 + i % 40 for i in range(B_DISTINCT)])
    return [base[i] for i in np.concatenate([np.arange(B_DISTINCT), rng.integers(0, B_DISTINCT, max(0, nq - B_DISTINCT))])[:nq]]


def b_case(dcp, cus):
    rng = np.random.default_rng(14100)
    profiles = pr.make_profiles(dcp, pr.make_params(rng, B_SPEC), B_SPEC)
    return profiles, b_queries(rng, b_nq(cus))


def b_w3_case(dcp, cus):
    """64 queries (the three-wavefront kernel) against enough flagged class-0 profiles of 3 .. 8 nodes for more than T
    redo pairs"""
    rng = np.random.default_rng(14150)
    nprof = T_of(1, cus) // 64 + 1
    spec = [-B_W3_SIZES[i % len(B_W3_SIZES)] for i in range(nprof)]
    return pr.make_profiles(dcp, pr.make_params(rng, spec), spec), b_queries(rng, 64)


def d_case(dcp, cus):
    """the {3, 4} class of B_SPEC alone, against enough queries for n > T redo pairs"""
    rng = np.random.default_rng(14200)
    spec = [m for m in B_SPEC if pr.class_of(abs(m)) == (3, 4)]
    nq = T_of(4, cus) // len(spec) + 1
    return pr.make_profiles(dcp, pr.make_params(rng, spec), spec), b_queries(rng, nq)


def test_b_shapes():
    cl = b_classes()
    assert {k: len(v) for k, v in cl.items()} == {(1, 1): 9, (8, 1): 9, (3, 4): 3}
    assert all(m < 0 for m in B_SPEC)
    for cus in CU_COUNTS:
        nq = b_nq(cus)
        assert all(len(v) * nq > T_of(W, cus) for (_, W), v in cl.items())
        assert any(len(v) * (nq - 1) <= T_of(W, cus) for (_, W), v in cl.items())  # the smallest such nq
        assert (T_of(1, cus) // 64 + 1) * 64 > T_of(1, cus)
    assert b_nq(256) == 911 and T_of(1, 256) // 64 + 1 == 129


def test_b_delete_states_decide_e(dcp, oracle32):
    """The premise of "every pair of a flagged profile is redone" is the upload's flag (positive MD / DD); that the
    flag is needed -- E(j) taken over the match states alone would change the score -- shows on the oracle's best
    path: for every flagged profile some query's path enters E from a delete state.  All scores are finite, as
    test_gpu_parity.test_positive_delete_transitions_keep_d_in_e asserts of its own."""
    rng = np.random.default_rng(14100)
    profiles = pr.make_profiles(dcp, pr.make_params(rng, B_SPEC), B_SPEC)
    seqs = pr.rand_of(np.random.default_rng(5), [6, 12, 21, 30, 40])
    for p, prof in enumerate(profiles):
        t8 = np.ascontiguousarray(prof.trans8, np.float32)
        assert prof.core_size >= 3 and (t8[[4, 5], 2:] > 0).all(), p  # DCP_T_MD, DCP_T_DD: the gains on M_1.. -> D, D -> D
        eps = tp.prof_eps[id(prof)]
        em = pr.host_table(dcp, prof)
        ei, en = dcp.frame_table_host(prof.insert_dist, eps), dcp.frame_table_host(prof.null_dist, eps)
        from_delete = 0
        for s in seqs:
            nl, al, (states, _), _ = oracle32.dp_tables_path(t8, em, ei, en, dcp.xtrans(len(s), True, False), bytes(s))
            assert np.isfinite(nl) and np.isfinite(al)
            st = states.tolist()
            from_delete += sum(1 for i, v in enumerate(st) if v == E_STATE and i and (st[i - 1] >> 14) == 2)
        assert from_delete > 0, (p, prof.core_size)


# ---- float, case C: seg_redo ---------------------------------------------------------------------------------------
C_SPEC = [513, (641, "eps0"), 768]


def c_case(dcp, cus):
    """three profiles of the {3, 4} class against enough queries of 1 .. 30 nt that the pairs of the two profiles with
    frame shifts alone -- E is finite in row 1 of each -- are more than 8 x CUs"""
    rng = np.random.default_rng(14300)
    profiles = pr.make_profiles(dcp, pr.make_params(rng, C_SPEC), C_SPEC)
    return profiles, pr.d_queries(rng, c_nq(cus), 30)


def c_nq(cus):
    return 8 * cus // 2 + 1


def c_seg_redo(seqs):
    """pairs that leave through seg_redo under "eb_only": all but the epsilon-0 profile's whose E is never finite"""
    return len(C_SPEC) * len(seqs) - sum(pr.e_never_finite_eps0(s) for s in seqs)


def test_c_shapes():
    assert {pr.class_of(pr.size_of(m)) for m in C_SPEC} == {(3, 4)}
    for cus in CU_COUNTS:
        n = len(C_SPEC) * c_nq(cus)
        assert 2 * c_nq(cus) > 8 * cus and seg_redo_blocks(n, cus) == 8 * cus
        assert trips(2 * c_nq(cus), 8 * cus) == 2 == trips(n, 8 * cus)


# ---- double --------------------------------------------------------------------------------------------------------
A64_SIZES = [257, 300, 513, 64, 128, 256]  # the segmented group, and one profile in each other group
A64_LMAX = 29_800  # seg_waves = 2^27 / (5 x 29 801) = 900
A64_SHORT = [1, 2, 3, 15, 16, 17, 33]
A64_N = ["sw-1", "sw", "sw+1", "2sw+3"]
A64_OTHER = {"sw-1": (1, 2, 3), "sw": (4, 5, 6), "sw+1": (7, 8, 9), "2sw+3": (9, 1, 5)}  # list lengths of groups 0, 1, 2
B64_SIZES = [64, 64, 64, 128, 128, 128, 256, 256, 256, 257, 280, 300]
X_NB, X_EB, X_JB = pr.X_NB, pr.X_EB, pr.X_JB


def a64_params():
    rng = np.random.default_rng(14400)
    return [tp.pfam_like_params(rng, M) for M in A64_SIZES]


def a64_queries():
    rng = np.random.default_rng(14401)
    return pr.rand_of(rng, A64_SHORT + [A64_LMAX])


def a64_lists(name):
    """{group: list} and the call's list; the long query (index len(A64_SHORT)) once, at position 0 of group 3's list,
    against the 257-node profile: wavefront 0's boundary column serves a short pair next"""
    sw = seg_waves(A64_LMAX, 10 ** 9)
    n3 = {"sw-1": sw - 1, "sw": sw, "sw+1": sw + 1, "2sw+3": 2 * sw + 3}[name]
    short = list(range(len(A64_SHORT)))
    combos = [(q, p) for q in short for p in (0, 1, 2)]
    per = {3: [(len(A64_SHORT), 0)] + [combos[(i * 5 + i // len(combos)) % len(combos)] for i in range(1, n3)]}
    for g, n in enumerate(A64_OTHER[name]):
        per[g] = [(short[(i * 3 + g) % len(short)], 3 + g) for i in range(n)]
    longest = max(len(v) for v in per.values())
    whole = [per[g][i] for i in range(longest) for g in sorted(per) if i < len(per[g])]
    return per, whole


def eb_only64(dcp, seqs):
    """E -> B and J -> B free, N -> B closed, the rest length-derived (multi-hit): [nseq, 13] in double"""
    xt = np.stack([dcp.xtrans64(len(s), True, False) for s in seqs])
    xt[:, X_EB] = 0.0
    xt[:, X_JB] = 0.0
    xt[:, X_NB] = -np.inf
    return xt


def b64_nq():
    return F64_REDO_WAVES // 3 + 1


def b64_params(sizes=B64_SIZES):
    rng = np.random.default_rng(14500)
    return [tp.pfam_like_params(rng, M) for M in sizes]


def b64_queries(nq):
    return b_queries(np.random.default_rng(14501), nq)


def host_tables64(dcp, oracle64, params):
    """(trans8, match [1364, M], insert, null tables) per profile in double, expanded by the oracle"""
    out = []
    for prm in params:
        prof = dcp.ProteinProfile.from_params(*prm, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01))), precision=64)
        t8, nd, idd, md = prof.parts64()
        eps = float(np.float32(0.01))
        out.append((t8, np.stack([oracle64.frame_table(md[k], eps) for k in range(prof.core_size)], axis=1),
                    oracle64.frame_table(idd, eps), oracle64.frame_table(nd, eps)))
    return out


def test_a64_lists_and_finite_scores(dcp, oracle64):
    assert [f64_group_of(M) for M in A64_SIZES] == [3, 3, 3, 0, 1, 2]
    sw = seg_waves(A64_LMAX, 10 ** 9)
    seen = set()
    for name in A64_N:
        per, whole = a64_lists(name)
        assert sorted(whole) == sorted(p for v in per.values() for p in v)
        assert per[3][0] == (len(A64_SHORT), 0) and sum(q == len(A64_SHORT) for q, _ in whole) == 1
        assert all(f64_group_of(A64_SIZES[p]) == g for g, v in per.items() for _, p in v)
        if len(per[3]) > sw:
            assert per[3][sw][0] < len(A64_SHORT)  # a short pair reuses wavefront 0's column
        seen |= {len(per[g]) for g in (0, 1, 2)}
    assert seen == set(range(1, 10))
    seqs = a64_queries()
    tabs = host_tables64(dcp, oracle64, a64_params())
    for q, s in enumerate(seqs):
        for p, (t8, em, ei, en) in enumerate(tabs):
            if len(s) == A64_LMAX and p != 0:
                continue  # listed against the 257-node profile only
            rc, nl, al = oracle64.dp_tables(t8, em, ei, en, dcp.xtrans64(len(s), True, False), bytes(s))
            assert rc == 0 and np.isfinite(nl) and np.isfinite(al) and np.isfinite(-2 * (nl - al)), (q, p)


def test_b64_every_pair_is_redone(dcp, oracle64):
    """With E -> B, J -> B free and N -> B closed every pair's alt score is finite and its best path passes E: B was
    entered at row 0 (S -> B) and E reached in some row j <= L, so E(j) + EB is finite there and beats N(j) + NB =
    -inf -- `fmax(E + x.EB, J + x.JB) > N + x.NB`, the f64 query-lane kernel's redo criterion, a comparison of the
    row's values.  (Whether the BEST path re-enters B is another matter: that of a 1-nt query cannot, and a short
    random query's often does not -- its single pass through the core already is the best path; so the GPU case rests
    on the values, and on dcp_gpu_last_scan_redo_pairs.)"""
    assert [f64_group_of(M) for M in B64_SIZES] == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert 3 * b64_nq() > F64_REDO_WAVES >= 3 * (b64_nq() - 1)
    seqs = b64_queries(B_DISTINCT)
    assert sorted({len(s) for s in seqs}) == list(range(1, 41))
    xt = eb_only64(dcp, seqs)
    tabs = host_tables64(dcp, oracle64, b64_params([64, 128, 256, 280]))
    for t8, em, ei, en in tabs:
        for q, s in enumerate(seqs):
            nl, al, (states, _), _ = oracle64.dp_tables_path(t8, em, ei, en, xt[q], bytes(s))
            assert np.isfinite(nl) and np.isfinite(al), (t8.shape[1], q)
            st = states.tolist()
            assert st.count(B_STATE) >= 1 and st.count(E_STATE) >= 1, (t8.shape[1], q)
