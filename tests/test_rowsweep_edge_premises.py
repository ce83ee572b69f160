"""The cases of tests/test_rowsweep_edges.py (families A .. D) and what they rest on, checked on the CPU.

The float row sweep's driver (launch_rowsweep_scan, dcp_gpu.hip) picks a code path from the batch size, the DB's
composition, the column budget and the scan's size.  Every case below is built for one such path; what can be known
without a device is asserted here:

  * the rule the shipped library applies to a batch size (rowsweep_variant), restated from the library's own
    dcp_rowsweep_max_block_waves / dcp_rowsweep_stage_bytes, gives the pinned table A_TRIPLES over family A's batch
    sizes, and changes where the driver's comments say (5 / 6, 36 / 37, 56 / 57);
  * family C's planted queries are what they are meant to be: on the oracle's float32 best path a two-copy query
    enters B at least twice (back to back: through E -> B; spaced: through J), a one-copy query once -- the float twin
    of test_f64_edges.test_planted_copies_reenter_b;
  * the median threshold of the GPU helper publishes between a quarter and three quarters of each case's finite pairs
    as hits, and every case has a pair with a non-finite LRT (NONFINITE says why not where it has none), with the
    oracle fed the host's expansion of the tables (the device's are the same values: expand_on_host, asserted by
    test_gpu_parity.oracle_dp_on_product_tables at upload).
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_parity as tp
from oracle_py import B_STATE, E_STATE, ENTRY_DIST_OCCUPANCY, J_STATE

MODES4 = [(True, False), (False, False), (True, True), (False, True)]
X_NB, X_EB, X_JB = 4, 9, 12  # RR SB SN NN NB ET EC CC CT EB EJ JJ JB
MP_CLASS1_MAX_QUERIES = 96  # kMpClass1MaxQueries


def class_of(M):
    """(R, W) of the row sweep's size class (kClasses)."""
    for R, W in [(r, 1) for r in range(1, 9)] + [(3, 4), (4, 4), (3, 8), (4, 8), (3, 16), (4, 16)]:
        if M <= 64 * R * W:
            return R, W
    raise ValueError(M)


def flagged_params(rng, M):
    """Positive MD / DD: a delete state decides E(j); the profile is flagged DCP_PROF_EXACT_E at upload."""
    null, match, trans = tp.pfam_like_params(rng, M)
    trans = trans.copy()
    trans[1:M, 2] = np.float32(0.7)
    trans[1:M, 6] = np.float32(0.4)
    return null, match, trans


def size_of(m):
    return abs(m[0] if isinstance(m, tuple) else m)


def is_flagged(m):
    return not isinstance(m, tuple) and m < 0


def make_params(rng, spec):
    """spec: core sizes; a negative one is a flagged profile, (M, "delete") a delete-heavy one, (M, "eps0") see
    make_profiles."""
    out = []
    for m in spec:
        if isinstance(m, tuple):
            out.append(tp.delete_heavy_params(rng, m[0]) if m[1] == "delete" else tp.pfam_like_params(rng, m[0]))
        else:
            out.append(flagged_params(rng, -m) if m < 0 else tp.pfam_like_params(rng, m))
    return out


def make_profiles(dcp, params, spec):
    """Epsilon 0.01, but 0 for an (M, "eps0") profile: without frame shifts only whole codons are emitted, so a query
    whose length is no multiple of 3 has null = alt = -inf and a NaN LRT -- every case's pairs with a non-finite LRT,
    which the filter must drop."""
    profiles = []
    for prm, m in zip(params, spec):
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0 if isinstance(m, tuple) and m[1] == "eps0" else 0.01)
        profiles.append(dcp.ProteinProfile.from_params(*prm, cfg))
        tp.prof_eps[id(profiles[-1])] = cfg.epsilon
    return profiles


def rand_of(rng, lens):
    return [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]


def host_table(dcp, prof):
    """The match table [1364, M] as expand_on_host uploads it."""
    eps = tp.prof_eps[id(prof)]
    md = prof.match_dist  # (a copy per access)
    return np.stack([dcp.frame_table_host(md[k], eps) for k in range(prof.core_size)], axis=1)


def mode_xtrans(dcp, seqs, mode):
    """[nseq, 13]: the length-derived special transitions of a (multi, h3) mode, or an explicit set by name."""
    if mode == "eb_free":
        xt = np.stack([dcp.xtrans(len(s), True, False) for s in seqs])
        xt[:, X_EB] = 0.0
    elif mode == "eb_only":  # E -> B free and N -> B closed: past row 0 B is entered from E (or J) alone
        xt = np.stack([dcp.xtrans(len(s), True, False) for s in seqs])
        xt[:, X_EB] = 0.0
        xt[:, X_NB] = -np.inf
    elif mode == "jb_free":
        xt = np.stack([dcp.xtrans(len(s), True, False) for s in seqs])
        xt[:, X_JB] = 0.0
    elif mode == "log1":
        xt = np.zeros((len(seqs), 13), np.float32)  # a profile that never saw protein_profile_setup
    else:
        xt = np.stack([dcp.xtrans(len(s), mode[0], mode[1]) for s in seqs])
    return xt.astype(np.float32)


def oracle_scores(dcp, oracle32, profiles, tables, seqs, xt):
    """test_gpu_parity.oracle_dp_on_product_tables' computation -- orc_dp_tables in float32 on the given match tables
    (the device's, or the host's expansion) -- with explicit special transitions xt [nseq, 13] and the profiles spread
    over threads (the C call releases the interpreter lock).  Identical queries are scored once."""
    nl = np.zeros((len(seqs), len(profiles)), np.float32)
    al = np.zeros_like(nl)
    keys = [bytes(s) + xt[q].tobytes() for q, s in enumerate(seqs)]
    first = {}
    for q, k in enumerate(keys):
        first.setdefault(k, q)
    src = np.array([first[k] for k in keys])

    args = []
    for p, prof in enumerate(profiles):
        eps = tp.prof_eps[id(prof)]
        args.append((np.ascontiguousarray(prof.trans8, np.float32), np.ascontiguousarray(tables[p], np.float32),
                     dcp.frame_table_host(prof.insert_dist, eps), dcp.frame_table_host(prof.null_dist, eps)))

    def one(pq):
        p, q = pq
        rc, nl[q, p], al[q, p] = oracle32.dp_tables(*args[p], xt[q], bytes(seqs[q]))
        assert rc == 0
    pairs = [(p, int(q)) for p in range(len(profiles)) for q in np.unique(src)]
    pairs.sort(key=lambda pq: -profiles[pq[0]].core_size * len(seqs[pq[1]]))  # the long ones first: even threads
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(one, pairs))
    return nl[src], al[src]


def median_filter(on, oa, q0, q1):
    """The helper's threshold and hit mask for a scan of [q0, q1): the median of the range's finite LRTs; a hit is
    isfinite(lrt) and not lrt < thr, lrt = float32(-2) * (null - alt) (scan_thread.c:121-123)."""
    with np.errstate(invalid="ignore"):
        lrt = np.float32(-2) * (on - oa)
    fin = np.isfinite(lrt[q0:q1])
    thr = np.sort(lrt[q0:q1][fin])[fin.sum() // 2] if fin.any() else np.float32(0)
    with np.errstate(invalid="ignore"):
        hit = np.isfinite(lrt) & ~(lrt < thr)
    hit[:q0], hit[q1:] = False, False
    return thr, hit, int(fin.sum())


def assert_filter_is_balanced(on, oa, q0, q1, what):
    thr, hit, nfin = median_filter(on, oa, q0, q1)
    if nfin >= 4:
        assert nfin / 4 <= hit.sum() <= 3 * nfin / 4 + 1, (what, int(hit.sum()), nfin)
    return nfin


# ---- family A: batch-size rules ------------------------------------------------------------------------------------
A_ENDS = [1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512]
# class 0 unflagged: 1, 64, 2, 3, 7, 30, 50 = a full group of four and one of three; class 1: 65, 128, 90 = a full group
# of two and a single; one flagged profile (class 0); 600 nodes: the {3, 4} class, four wavefronts per pair
A_SIZES = A_ENDS + [2, 3, 7, (30, "eps0"), 50, 90, -40, 600]
A_LENGTHS = list(range(1, 46)) * 2 + list(range(1, 14))  # 103 queries: every tail of the five- and ten-row unrolling
A_NQ = list(range(1, 65)) + [65, 70, 95, 96, 97, 100]
A_Q0 = (0, 3)
# the (stage, waves, prefetch) triples rowsweep_variant gives the one-wavefront classes R = 2 .. 8 over A_NQ (R = 2 from
# 96 queries on, below it runs K profiles per wavefront; R = 1 always does).  Pinned: a change of the rule shows up here
# (test_a_pinned_triples) before the GPU cases run.
A_TRIPLES = ([(20, w, 1) for w in (1, 2, 3, 4, 5, 6, 7, 8)] + [(20, w, 0) for w in (4, 7, 8)] +
             [(84, w, 1) for w in range(5, 17)])


def a_case(dcp):
    rng = np.random.default_rng(13001)
    profiles = make_profiles(dcp, make_params(rng, A_SIZES), A_SIZES)
    seqs = rand_of(rng, rng.permutation(A_LENGTHS))
    return profiles, seqs


def balanced(nq, maxw):
    nb = -(-nq // maxw)
    return -(-nq // nb)


def shipped_variant(lib, R, W, nq):
    """rowsweep_variant (dcp_gpu.hip) with nothing forced: (stage, waves, prefetch)."""
    if W != 1:
        return 0, 1, 0
    g, w = 20, balanced(nq, 8 if nq <= 56 else 4)
    max84 = lib.dcp_rowsweep_max_block_waves(R, W, 84)
    if 6 <= nq <= 36 and max84:
        w84 = balanced(nq, max84)
        blocks = (160 * 1024) // lib.dcp_rowsweep_stage_bytes(R, 84)
        if min(blocks * w84, max84) * 2 >= max84:
            g, w = 84, w84
    return g, max(1, w), int(nq <= 36)


def a_expected_plan(lib, nq):
    """{(R, W): path or (stage, waves, prefetch)} of family A's DB for a scan of nq queries by the shipped rule."""
    plan = {(1, 1): "mp", (2, 1): "mp" if nq < MP_CLASS1_MAX_QUERIES else shipped_variant(lib, 2, 1, nq)}
    for R in range(3, 9):
        plan[(R, 1)] = shipped_variant(lib, R, 1, nq)
    plan[(3, 4)] = (0, 1, 0)
    return plan


def a_triples(lib):
    return sorted({t for nq in A_NQ for t in a_expected_plan(lib, nq).values() if t != "mp" and t != (0, 1, 0)})


def product_lib(dcp):
    lib = C.CDLL(dcp.LIB_PATH)
    lib.dcp_rowsweep_max_block_waves.restype = C.c_uint
    lib.dcp_rowsweep_max_block_waves.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.dcp_rowsweep_stage_bytes.restype = C.c_uint
    lib.dcp_rowsweep_stage_bytes.argtypes = [C.c_int, C.c_int]
    return lib


def test_a_pinned_triples(dcp):
    lib = product_lib(dcp)
    assert a_triples(lib) == sorted(A_TRIPLES)
    for R in range(2, 9):
        by_nq = {nq: shipped_variant(lib, R, 1, nq) for nq in range(1, 101)}
        # prefetch ends at 36; stage 84 only inside 6 .. 36 (R = 8 has no 84-row kernel: 172 KB of LDS)
        assert all(v[2] == int(nq <= 36) for nq, v in by_nq.items())
        assert all(v[0] == 20 for nq, v in by_nq.items() if nq < 6 or nq > 36)
        if R == 8:
            assert all(v[0] == 20 for v in by_nq.values())
        # the 20-row image: blocks of equal width, at most 8 wavefronts up to 56 queries and 4 beyond
        assert all(v[1] == balanced(nq, 8 if nq <= 56 else 4) for nq, v in by_nq.items() if v[0] == 20)
        assert by_nq[56][1] == 8 and by_nq[57][1] == 4
    # some class takes the 84-row image at both ends of its range, none past them
    assert any(shipped_variant(lib, R, 1, 6)[0] == 84 for R in range(2, 9))
    assert any(shipped_variant(lib, R, 1, 36)[0] == 84 for R in range(2, 9))
    # every width from 1 to 8 occurs, and blocks that are not full (the width does not divide nq)
    widths = {v[1] for nq in A_NQ for v in [shipped_variant(lib, 5, 1, nq)]}
    assert set(range(1, 9)) <= widths
    assert any(nq % shipped_variant(lib, 5, 1, nq)[1] for nq in A_NQ)


# ---- family B: group compositions ----------------------------------------------------------------------------------
# name -> core sizes in upload order (negative: flagged).  K = 4 in class 0 (<= 64 nodes), K = 2 in class 1 (65 .. 128).
B_DBS = {
    "c0_empty_c1_grouped": [65, 100, 128],                      # mp_first[1] < mp_first[0]: the fix-up lines
    "c1_empty": [1, 5, 64, 33, 20, 200],
    "c0_flagged_only": [-40, -9, 65, 127],                      # use_mp false in class 0: the generic variant on column views
    "c1_flagged_only": [3, 64, 17, 50, 8, -100],
    "flagged_only_both": [-40, -100, -64, -65],
    "exactly_k": [4, 16, 61, 64, 66, 128],
    "k_plus_1": [4, 16, 61, 64, 9, 66, 128, 97],
    "two_k_minus_1": [4, 16, 61, 64, 9, 10, 11, 66, 128, 97],
    "m_mod_4": [64, 5, 6, 7, 61, 62, 63, 128, 65, 66, 67, 125, 126, 127],
    "flagged_between": [10, -40, 20, 70, -100, 80],
}
B_RANGES = [(0, 1), (0, 4), (0, 5), (0, 21), (3, 24)]  # nq = 1, 4, 5, 21 and a ranged scan of 21 from query 3
B_LENGTHS = list(range(1, 22)) + [30, 2, 11]


def b_spec(name):
    """The composition, its first unflagged profile (or its first) at epsilon 0."""
    spec = list(B_DBS[name])
    i = next((i for i, m in enumerate(spec) if m > 0), None)
    if i is not None:
        spec[i] = (spec[i], "eps0")
    return spec


def b_case(dcp, name):
    rng = np.random.default_rng(13100 + sorted(B_DBS).index(name))
    spec = b_spec(name)
    profiles = make_profiles(dcp, make_params(rng, spec), spec)
    seqs = rand_of(rng, rng.permutation(B_LENGTHS))
    return profiles, seqs


def b_expected_paths(name):
    """{(R, W): (path, flagged_rest)}: a class of at most 128 nodes runs K profiles per wavefront iff it has an
    unflagged member; its flagged members then get the one-profile kernel's launch."""
    out = {}
    for R in (1, 2):
        mine = [m for m in B_DBS[name] if class_of(abs(m)) == (R, 1)]
        if mine:
            grouped = any(m > 0 for m in mine)
            out[(R, 1)] = ("mp", any(m < 0 for m in mine)) if grouped else ("plain", False)
    for m in B_DBS[name]:
        if abs(m) > 128:
            out[class_of(abs(m))] = ("plain", False)
    return out


def test_b_compositions():
    """The compositions are what their names say (group sizes by the upload rule: unflagged members of a class in
    upload order, K to a group)."""
    def members(name, R):
        return [m for m in B_DBS[name] if class_of(abs(m)) == (R, 1) and m > 0]
    assert members("c0_empty_c1_grouped", 1) == [] and len(members("c0_empty_c1_grouped", 2)) == 3
    assert members("c1_empty", 2) == [] and not [m for m in B_DBS["c1_empty"] if class_of(abs(m)) == (2, 1)]
    assert members("c0_flagged_only", 1) == [] and members("c1_flagged_only", 2) == []
    assert members("flagged_only_both", 1) == [] and members("flagged_only_both", 2) == []
    for name, k0, k1 in (("exactly_k", 4, 2), ("k_plus_1", 5, 3), ("two_k_minus_1", 7, 3)):
        assert (len(members(name, 1)), len(members(name, 2))) == (k0, k1)
    assert {m % 4 for m in members("m_mod_4", 1)} == {0, 1, 2, 3} == {m % 4 for m in members("m_mod_4", 2)}
    assert B_DBS["flagged_between"][:3] == [10, -40, 20] and B_DBS["flagged_between"][3:] == [70, -100, 80]
    assert b_expected_paths("c0_flagged_only") == {(1, 1): ("plain", False), (2, 1): ("mp", False)}
    assert b_expected_paths("flagged_between") == {(1, 1): ("mp", True), (2, 1): ("mp", True)}


# ---- family C: segments and chunks ---------------------------------------------------------------------------------
# two profiles at the ends of every multi-wavefront class; 2500 and 3072: one lane width (8 nodes), five and six
# segments; a delete-heavy and a flagged profile (both in the {3, 4} class)
C_SIZES = [513, 768, (769, "eps0"), 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073, 4096, 2500, (700, "delete"), -640]
C_PLANT = (513, 1025)  # two and three segments
C_LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 19, 20, 21, 33, 47, 64, 65, 100, 120]
C_CHUNKS = (1, 3, 4, 5, "nq-1", "nq", "more")
C_MODES = MODES4 + ["eb_free", "eb_only", "jb_free", "log1"]
_c = {}


def seg_r_of(M):
    nseg = -(-M // 512)
    return -(-M // (64 * nseg))


def nseg_of(M):
    return -(-M // (64 * seg_r_of(M)))


def c_case(dcp, oracle32):
    """(profiles, seqs, planted): 23 random queries of 1 .. 120 nt and, scattered among them, one-copy, back-to-back
    two-copy and spaced two-copy queries of the planted cores of the 513- and the 1025-node profile.
    planted = [(query index, profile index, copies, spaced)]."""
    if _c:
        return _c["v"]
    rng = np.random.default_rng(13200)
    params = make_params(rng, C_SIZES)
    profiles = make_profiles(dcp, params, C_SIZES)
    seqs = rand_of(rng, rng.permutation(C_LENGTHS))
    planted = []
    for M in C_PLANT:
        p = C_SIZES.index(M)
        op = oracle32.new(*params[p], ENTRY_DIST_OCCUPANCY, 0.01)
        core = tp.planted_query(rng, op, M, flank=0)
        for copies, spaced in ((1, False), (2, False), (2, True)):
            parts = [rng.integers(0, 4, 3, dtype=np.uint8), core]
            if copies == 2:
                if spaced:
                    parts.append(rng.integers(0, 4, 40, dtype=np.uint8))
                parts.append(core)
            parts.append(rng.integers(0, 4, 3, dtype=np.uint8))
            at = int(rng.integers(0, len(seqs) + 1))
            seqs.insert(at, np.concatenate(parts))
            planted = [(q + (q >= at), pp, c, s) for q, pp, c, s in planted] + [(at, p, copies, spaced)]
        _c[M] = op
    _c["v"] = (profiles, seqs, planted)
    return _c["v"]


def e_never_finite_eps0(seq):
    """Against a profile of epsilon 0, with N -> B closed: E(j) is -inf in every row iff the query has no first codon
    or it is a stop codon (TAA, TAG, TGA: no amino acid, so no match state emits it; every other codon has a positive
    probability in every match state, and B(0) -> M_k -> E exits from any node)."""
    return len(seq) < 3 or tuple(int(x) for x in seq[:3]) in ((3, 0, 0), (3, 0, 2), (3, 2, 0))


def c_ranges(nq):
    return [(0, nq), (2, 17), (9, nq)]  # query 2 lies inside the whole batch's first chunk of 3, 4 or 5


def c_class_counts():
    out = {}
    for m in C_SIZES:
        k = class_of(size_of(m))
        n, f = out.get(k, (0, 0))
        out[k] = (n + 1, f + is_flagged(m))
    return out  # (R, W) -> (profiles, flagged among them)


def c_budget(target, lens):
    """Bytes of boundary columns (plan_segsweep: np x chunk pairs x 2 columns x stride rows x 16 bytes within the cap,
    stride = the range's longest query + 2) that give a class of TWO profiles `target` queries per chunk."""
    return target * 2 * 2 * (max(lens) + 2) * 16


def c_expected_chunks(budget, lens):
    """{(R, W): chunk} by plan_segsweep's formula; 0: the budget holds no query of the class, which is then not swept in
    segments."""
    nq, stride = len(lens), max(lens) + 2
    return {k: min(nq, budget // (n * 2 * stride * 16)) for k, (n, _) in c_class_counts().items()}


def test_c_db_and_budgets(dcp, oracle32):
    profiles, seqs, planted = c_case(dcp, oracle32)
    assert len(seqs) == len(C_LENGTHS) + 6 and len(C_LENGTHS) == 23
    assert sorted(c_class_counts()) == [(3, 4), (3, 8), (3, 16), (4, 4), (4, 8), (4, 16)]
    assert (seg_r_of(2500), nseg_of(2500)) == (8, 5) and (seg_r_of(3072), nseg_of(3072)) == (8, 6)
    assert class_of(2500) == class_of(3072)
    assert [nseg_of(M) for M in C_PLANT] == [2, 3]
    lens = [len(s) for s in seqs]
    nq = len(seqs)
    for q0, q1 in c_ranges(nq):
        sub = lens[q0:q1]
        for target in C_CHUNKS:
            t = {"nq-1": len(sub) - 1, "nq": len(sub), "more": len(sub) + 5}.get(target, target)
            chunks = c_expected_chunks(c_budget(t, sub), sub)
            assert chunks[(4, 4)] == min(t, len(sub))  # the classes of two profiles get the target
            assert chunks[(3, 4)] == min(t // 2, len(sub))  # four profiles: half of it (at 1: none, the exact kernel)
    # the second range starts inside a chunk of the whole batch's scan for chunks of 3, 4, 5
    assert all(2 % c for c in (3, 4, 5))


def test_c_planted_copies_reenter_b(dcp, oracle32):
    """On the oracle's float32 best path (multi-hit) a two-copy query enters B at least twice -- back to back through
    E -> B, spaced through J -- and a one-copy query exactly once: the segmented sweep's B(j) = N(j) + NB is wrong
    for the former, which must leave through seg_redo."""
    profiles, seqs, planted = c_case(dcp, oracle32)
    assert sorted((c, s) for _, _, c, s in planted) == sorted([(1, False), (2, False), (2, True)] * 2)
    for q, p, copies, spaced in planted:
        op = _c[profiles[p].core_size]
        op.setup(len(seqs[q]), True, False)
        rc, ll, path = op.viterbi(1, bytes(seqs[q]))
        assert rc == 0 and np.isfinite(ll)
        states = [s for s, _ in path]
        nb = states.count(B_STATE)
        if copies == 1:
            assert nb == 1, (q, p, nb)
            continue
        assert nb >= 2, (q, p, spaced, nb)
        into_b = [states[i - 1] for i, s in enumerate(states) if s == B_STATE and i > 0]
        if spaced:
            assert J_STATE in into_b, (q, p, into_b)
        else:
            assert E_STATE in into_b, (q, p, into_b)


# ---- family D: the shipped rules at scale --------------------------------------------------------------------------
D1_SIZES = [513, 640, (641, "eps0"), 768]
D2_SOURCES = [1, 2, (3, "eps0"), 4, 5, 6, 7, 8] + [65, 66, 67, 70, 77, 80, 85, 90, 95, 96, 97, 100, 105, 110, 115, 120, 125, 126, 127, 128] + D1_SIZES
D2_NPROF, D2_NQ = 2048, 2048  # (4096 x 1024 took 17 s, most of it the upload and the read-back of 4096 tables)


def d_queries(rng, nq, lmax):
    """nq queries of 1 .. lmax nt: copies of 64 distinct ones, in a random order."""
    base = rand_of(rng, [1 + i % lmax for i in range(64)])
    return [base[i] for i in np.concatenate([np.arange(64), rng.integers(0, 64, max(0, nq - 64))])[:nq]]


def d1_nq(cus):
    """One below and exactly at pairs = 16 x CUs with four profiles in the class."""
    at = -(-16 * cus // 4)
    return at - 1, at


def test_d_shapes():
    assert len(D2_SOURCES) == 32 and D2_NPROF * D2_NQ == 1 << 22
    assert {class_of(size_of(m)) for m in D1_SIZES} == {(3, 4)}
    for cus in (256, 304, 128):
        below, at = d1_nq(cus)
        assert 4 * below < 16 * cus <= 4 * at
    # D2: the {3, 4} class has 256 profiles x 2048 queries, far past 16 x CUs; class 1 has 96 or more queries
    assert D2_NPROF // 32 * 4 * D2_NQ >= 16 * 1024 and D2_NQ >= MP_CLASS1_MAX_QUERIES


# ---- the filter on every case --------------------------------------------------------------------------------------
# cases without a non-finite LRT, and why
NONFINITE = {"B/flagged_only_both": "the DB holds flagged profiles only; their gains on MD / DD keep every score finite"}


def check_filter_case(dcp, oracle32, what, profiles, seqs, modes, ranges):
    tables = [host_table(dcp, p) for p in profiles]
    assert modes
    for mode in modes:
        xt = mode_xtrans(dcp, seqs, mode)
        on, oa = oracle_scores(dcp, oracle32, profiles, tables, seqs, xt)
        assert not np.isnan(on).any() and not np.isnan(oa).any()
        for q0, q1 in ranges:
            nfin = assert_filter_is_balanced(on, oa, q0, q1, (what, mode, q0, q1))
            if q1 - q0 == len(seqs):
                assert (nfin < (q1 - q0) * len(profiles)) == (what not in NONFINITE), (what, mode)


def test_filter_family_a(dcp, oracle32):
    profiles, seqs = a_case(dcp)
    ranges = [(q0, q0 + nq) for nq in A_NQ for q0 in A_Q0] + [(0, len(seqs))]
    check_filter_case(dcp, oracle32, "A", profiles, seqs, MODES4, ranges)


@pytest.mark.parametrize("name", sorted(B_DBS))
def test_filter_family_b(dcp, oracle32, name):
    profiles, seqs = b_case(dcp, name)
    check_filter_case(dcp, oracle32, "B/" + name, profiles, seqs, MODES4, B_RANGES + [(0, len(seqs))])


def test_filter_family_c(dcp, oracle32):
    """Two of the seven modes: C's 6e8 oracle cells per mode are most of this file's time.  The GPU helper asserts the
    same bounds on every mode's scores."""
    profiles, seqs, _ = c_case(dcp, oracle32)
    check_filter_case(dcp, oracle32, "C", profiles, seqs, [(True, False), "eb_free"], c_ranges(len(seqs)))


def test_filter_family_d(dcp, oracle32):
    """D1 and D2 on their distinct queries x source profiles (the copies change no fraction by more than their share:
    the GPU helper asserts the same bounds on the full case)."""
    for spec, lmax in ((D1_SIZES, 30), (D2_SOURCES, 6)):
        rng = np.random.default_rng(13300)
        profiles = make_profiles(dcp, make_params(rng, spec), spec)
        seqs = d_queries(rng, 64, lmax)
        check_filter_case(dcp, oracle32, "D", profiles, seqs, [(True, False), (False, True)], [(0, 64)])
