"""The float row sweep (viterbi_rowsweep_kernel, viterbi_mp_kernel, viterbi_segment_kernel and their driver
launch_rowsweep_scan) at its batch, group, segment and chunk edges, one family of cases per edge (runs on a real MI355X).

Every case goes through ONE helper (check_case), so none is weaker than another: for every scoring mode of the case,
KERNEL_ROWSWEEP gives `null` and `alt` of EVERY pair of the scanned range equal, as uint32, to the oracle's float32
recursion fed the device's own tables (orc_dp_tables, as test_gpu_parity.oracle_dp_on_product_tables calls it; here
through test_rowsweep_edge_premises.oracle_scores, which spreads the pairs over threads and takes explicit special
transitions), and the hit list equals the reference's filter on those scores (isfinite(lrt) and not lrt < thr,
lrt = float32(-2) * (null - alt)) record for record, scores in bits, seq_idx the RESIDENT index.  The threshold is the
median of the range's finite LRTs, so about half of the pairs are hits (asserted: a quarter to three quarters).  No
score is NaN; every DB holds a profile of epsilon 0, whose pairs with queries of no whole number of codons have
null = alt = -inf, a NaN LRT, and must not be hits.  Nothing is sampled; the oracle is computed once per (DB, batch,
mode) and every ranged scan of the batch is compared with a slice of it.

Which path a scan took is asserted from the test-hooks build's read-only dcp_gpu_test_last_rowsweep_plan
(Scanner.test_rowsweep_plan) and from the launch list; what the shipped rule should choose is restated, and checked
on the CPU, in test_rowsweep_edge_premises.

edge (dcp_gpu.hip unless said)                                       read from                      reached by
  stage 20 / 84 and prefetch at 5 / 6, 36 / 37 queries               rowsweep_variant: `nchunks >=   A: nq = 1 .. 64, 65, 70, 95, 96,
                                                                      6u && nchunks <= 36u`, `*pf`   97, 100 at q0 = 0 and 3
  block width balanced(8 | 4 | max84) = 1 .. 8, 9 .. 16; width cap   rowsweep_variant: `balanced(     A (the plan of every nq equals the
  at 56 / 57; a last block that is not full                           nchunks <= 56u ? 8u : 4u)`     rule's; pinned triples)
  class 1 leaves the K-profile kernel at 96 queries                  launch_rowsweep_scan: `nq <     A: nq = 95, 96, 97
                                                                      kMpClass1MaxQueries`
  hit record's `a.q_base + q` in viterbi_mp_kernel                   dcp_kernels.hip: `dcp_hit{a.q   A, B: ranged scans from q0 = 3
                                                                      _base + q, pidx, nul, alt}`
  class 0 empty, class 1 grouped (mp_first fix-up)                   upload: `if (c->mp_first[1] <   B c0_empty_c1_grouped
                                                                      c->mp_first[0])`
  a class of flagged profiles only: use_mp false, generic variant    launch_rowsweep_scan: `c->mp_   B c0_flagged_only, c1_flagged_only,
  on column views; in both classes                                    first[k + 1] > c->mp_first[k]` flagged_only_both
  groups of exactly K, K + 1, 2K - 1 members; M mod 4 = 1, 2, 3      upload: `while (members <       B exactly_k, k_plus_1, two_k_minus_1,
  beside 64 and 128; a flagged profile between two unflagged ones     kMpParts[k0] && ...`           m_mod_4, flagged_between
  segmented sweep: chunk loop seg_q0 / seg_nq = min(chunk, nq - qc), launch_segsweep_class: `for     C: budgets for chunks of 1, 3, 4, 5,
  four queries per block, chunk = 1 .. nq and more                    (unsigned qc = 0; qc < nq;`    nq - 1, nq, nq + 5 (a class of four
                                                                                                     profiles gets half, at 1: none)
  segmented x ranged scan (q_begin != 0, stride = lmax + 2 of the    plan_segsweep: `sp.stride =`    C: ranges (2, 17) and (9, nq): the first
  range; `a.q_base + q` in viterbi_segment_kernel)                                                   starts inside a chunk of the whole batch
  segmented x uni-hit, hmmer3_compat                                                                 C: all four (multi, h3)
  segmented x explicit transitions: E -> B free, with N -> B closed  dcp_kernels.hip: `sp.c = x ==  C: eb_free, log1, jb_free; eb_only
  (every pair leaves through seg_redo), J -> B free, LOG1 defaults    0u ? xt[DCP_X_NB] : ni`, `cJ`  (seg_redo = all pairs, from the hook)
  profiles of one lane width with different segment counts           launch_segsweep_class: `nseg_   C: 2500 and 3072 nodes (five and six
                                                                      max`; kernel: `seg >= nseg`    segments of 8 nodes per lane)
  segmentation switches on at pairs >= 16 x CUs                      plan_segsweep: `pairs >= 16ull  D1: four profiles x (4 x CUs - 1) and
                                                                      * c->num_cus`                  4 x CUs queries
  one stream from 2^22 pairs on (forked below)                       launch_rowsweep_scan: `overlap  D2: 4096 profiles x 1024 queries, then
                                                                      = ... < ((uint64_t)1 << 22)`   x 1023
"""
import time

import numpy as np
import pytest
import torch  # before the product's library: both bring a HIP runtime, and torch must see the device too

import test_gpu_parity as tp
import test_rowsweep_edge_premises as pr

pytestmark = pytest.mark.gpu

MODES2 = [(True, False), (False, True)]
PAIRS = {}  # family -> pairs compared against the oracle, printed per test
SEG_ON, SEG_OFF = 2 << 24, 1 << 24  # bits 24..25 of test_set_rowsweep_variant: the segmented sweep always / never


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def hooks_scanner(dcp):
    s = dcp.Scanner(0, lib=dcp.load_testhooks())
    yield s
    s.close()


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def mode_id(m):
    return m if isinstance(m, str) else "multi%d-h3%d" % m


class Case:
    """One DB and one resident batch; the oracle's scores per mode are computed once and kept."""

    def __init__(self, family, profiles, seqs, prof_src=None, on_host=True):
        self.family, self.profiles, self.seqs, self.on_host = family, profiles, seqs, on_host
        self.prof_src = np.arange(len(profiles)) if prof_src is None else np.asarray(prof_src)
        self.tables, self.scores = None, {}


_resident = {}  # id(scanner) -> the Case whose DB it holds (every upload of this file goes through check_case)


def upload(dcp, sc, case):
    """The DB, expanded on the host (or, D2, on the device); the device's tables of the distinct profiles, each copy's
    asserted equal to its source's and -- host expansion -- the source's ends to the host's values."""
    if _resident.get(id(sc)) is case:
        return
    sc.upload_db(case.profiles, expand_on_host=case.on_host)
    _resident[id(sc)] = case
    src = case.prof_src
    up = np.unique(src)
    assert np.array_equal(up, np.arange(len(up)))  # the sources come first
    tabs = [sc.match_table(int(p)) for p in up]
    for p in np.nonzero(src != np.arange(len(src)))[0]:
        assert np.array_equal(u32(sc.match_table(int(p))), u32(tabs[src[p]])), (int(p), int(src[p]))
    for p in up if case.on_host else []:
        prof = case.profiles[p]
        md = prof.match_dist
        for k in (0, prof.core_size - 1):
            assert np.array_equal(u32(tabs[p][:, k]), u32(dcp.frame_table_host(md[k], tp.prof_eps[id(prof)])))
    if case.tables is None:
        case.tables = tabs
    else:  # another context of the same DB: the oracle's scores hold for it if its tables are the same bits
        assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(tabs, case.tables))


def check_case(dcp, oracle32, sc, case, mode, ranges, after_scan=None):
    """The one check of this file (module docstring): `case` under `mode` -- (multi, h3), or the name of a set of
    explicit special transitions (pr.mode_xtrans) -- scanned over each (q0, q1) of `ranges`.  after_scan(q0, q1) runs
    behind each scan's own assertions (plans, launches).  Returns {(q0, q1): (null, alt, hits)} of the ranges."""
    upload(dcp, sc, case)
    seqs, src = case.seqs, case.prof_src
    nprof = len(case.profiles)
    sc.upload_seqs(seqs)  # (also returns to length-derived transitions)
    xt = pr.mode_xtrans(dcp, seqs, mode)
    if isinstance(mode, str):
        sc.set_xtrans(xt)
        flags = (True, False)  # ignored once explicit transitions are in force
    else:
        flags = mode
    if mode not in case.scores:
        uprofs = [case.profiles[p] for p in np.unique(src)]
        on, oa = pr.oracle_scores(dcp, oracle32, uprofs, case.tables, seqs, xt)
        assert not np.isnan(on).any() and not np.isnan(oa).any()
        case.scores[mode] = (on[:, src], oa[:, src])
    on, oa = case.scores[mode]
    out = {}
    for q0, q1 in ranges:
        what = "%s %s range (%d, %d)" % (case.family, mode_id(mode), q0, q1)
        thr, hit, nfin = pr.median_filter(on, oa, q0, q1)
        pr.assert_filter_is_balanced(on, oa, q0, q1, what)
        if (q0, q1) == (0, len(seqs)):
            assert (nfin < len(seqs) * nprof) == (case.family not in pr.NONFINITE), what
        wq, wp = np.nonzero(hit)  # row-major: sorted by (seq_idx, profile_idx) like dcp_gpu_fetch_hits
        sc.scan(flags[0], flags[1], float(thr), keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP, q_range=(q0, q1))
        assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP and sc.last_scan_redo_pairs == 0
        gn, ga = sc.scores()
        gn, ga = gn[q0:q1], ga[q0:q1]
        assert not np.isnan(gn).any() and not np.isnan(ga).any(), what
        bad = np.argwhere((u32(gn) != u32(on[q0:q1])) | (u32(ga) != u32(oa[q0:q1])))
        if len(bad):
            q, p = int(bad[0][0]) + q0, int(bad[0][1])
            raise AssertionError("%s: %d of %d pairs differ; first: query %d (L = %d) profile %d (M = %d): device null %r alt "
                                 "%r, oracle %r %r" % (what, len(bad), (q1 - q0) * nprof, q, len(seqs[q]), p,
                                                       case.profiles[p].core_size, gn[q - q0, p], ga[q - q0, p], on[q, p], oa[q, p]))
        hits = sc.hits()
        same = len(hits) == len(wq) and np.array_equal(hits["seq_idx"], wq) and np.array_equal(hits["profile_idx"], wp) \
            and np.array_equal(u32(hits["null_loglik"]), u32(on[wq, wp])) and np.array_equal(u32(hits["alt_loglik"]), u32(oa[wq, wp]))
        if not same:
            got = set(zip(hits["seq_idx"].tolist(), hits["profile_idx"].tolist()))
            diff = sorted(got ^ set(zip(wq.tolist(), wp.tolist())))
            raise AssertionError("%s: hit list differs (%d records, %d wanted, threshold %r); first (query, profile) in one list "
                                 "only: %r" % (what, len(hits), len(wq), thr, diff[0] if diff else None))
        if after_scan:
            after_scan(q0, q1)
        out[(q0, q1)] = (gn.copy(), ga.copy(), hits.copy())
        PAIRS[case.family[0]] = PAIRS.get(case.family[0], 0) + (q1 - q0) * nprof
    print("%s: %d pairs against the oracle so far" % (case.family[0], PAIRS[case.family[0]]))
    return out


def launches_per_class(sc):
    n = {}
    for li in sc.launch_infos():
        n[(li["R"], li["W"])] = n.get((li["R"], li["W"]), 0) + 1
    return n


# ---- A: the batch-size rules of the shipped choice -----------------------------------------------------------------
_cases = {}


def the_case(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


@pytest.mark.parametrize("mode", pr.MODES4, ids=mode_id)
@pytest.mark.parametrize("lib", ["shipped", "hooks"])
def test_a_batch_sizes(dcp, oracle32, scanner, hooks_scanner, lib, mode):
    """One DB -- a profile at each end of every one-wavefront class, a full and a partial group in classes 0 and 1, a
    flagged profile, 600 nodes -- against ranges of 1 .. 64, 65, 70, 95, 96, 97, 100 of 103 resident queries of 1 .. 45
    nt, from query 0 and from query 3.  The shipped library carries the assertion on bits; the test-hooks build with
    nothing forced must give the same and reports the plan of every nq: K profiles per wavefront in class 0 always (its
    flagged profile in a launch of the one-profile kernel) and in class 1 below 96 queries exactly, elsewhere the
    (stage, waves, prefetch) of rowsweep_variant as test_rowsweep_edge_premises restates and pins it."""
    case = the_case("A", lambda: Case("A", *pr.a_case(dcp)))
    sc = scanner if lib == "shipped" else hooks_scanner
    plib = pr.product_lib(dcp)
    seen = set()

    def after(q0, q1):
        nq = q1 - q0
        # every class is one launch: nothing is segmented below 16 x CUs pairs
        assert set(launches_per_class(sc).values()) == {1}
        if lib != "hooks":
            return
        plan = sc.test_rowsweep_plan()
        assert plan["forked"]
        want = pr.a_expected_plan(plib, nq)
        assert set(plan["classes"]) == set(want)
        for k, w in want.items():
            got = plan["classes"][k]
            if w == "mp":
                assert got["path"] == "mp" and got["flagged_rest"] == (k == (1, 1)), (nq, k, got)
            else:
                assert got["path"] == "plain" and (got["stage"], got["waves"], got["prefetch"]) == w, (nq, k, got, w)
                if k[1] == 1:
                    seen.add(w)
        assert (plan["classes"][(2, 1)]["path"] == "mp") == (nq < 96)
    ranges = [(q0, q0 + nq) for nq in pr.A_NQ for q0 in pr.A_Q0]
    check_case(dcp, oracle32, sc, case, mode, ranges, after)
    if lib == "hooks":
        assert seen == set(pr.A_TRIPLES)


# ---- B: group compositions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pr.B_DBS))
def test_b_group_compositions(dcp, oracle32, scanner, hooks_scanner, name):
    """Small DBs whose classes of at most 128 nodes are empty, flagged only, or hold exactly K, K + 1, 2K - 1 unflagged
    members (pr.B_DBS), scanned over 1, 4, 5, 21 queries and a range of 21 from query 3 in all four modes, on both
    builds; the hook says which kernel each class ran."""
    case = the_case("B/" + name, lambda: Case("B/" + name, *pr.b_case(dcp, name)))
    want = pr.b_expected_paths(name)

    def after(q0, q1):
        plan = hooks_scanner.test_rowsweep_plan()
        got = {k: (v["path"], v["flagged_rest"]) for k, v in plan["classes"].items()}
        assert got == want and plan["forked"], (name, got, want)
    for mode in pr.MODES4:
        a = check_case(dcp, oracle32, hooks_scanner, case, mode, pr.B_RANGES, after)
        b = check_case(dcp, oracle32, scanner, case, mode, pr.B_RANGES)
        assert all(np.array_equal(a[r][2], b[r][2]) for r in a)


# ---- D: the shipped rules at scale ---------------------------------------------------------------------------------
def copies_case(dcp, family, spec, nprof, nq, lmax, seed, on_host=True):
    rng = np.random.default_rng(seed)
    base = pr.make_profiles(dcp, pr.make_params(rng, spec), spec)
    src = np.concatenate([np.arange(len(base)), np.arange(nprof - len(base)) % len(base)])
    return Case(family, [base[i] for i in src], pr.d_queries(rng, nq, lmax), src, on_host)


@pytest.mark.parametrize("mode", MODES2, ids=mode_id)
def test_d1_segmentation_threshold(dcp, oracle32, scanner, hooks_scanner, mode):
    """Four profiles of the {3, 4} class (513, 640, 641, 768 nodes) against one query fewer than, and exactly,
    ceil(16 x CUs / 4) -- the shipped rule sweeps a class in segments from 16 x CUs pairs on: one launch below, two at
    it, on both builds; the hook names the path."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    below, at = pr.d1_nq(cus)
    case = the_case("D1", lambda: copies_case(dcp, "D1", pr.D1_SIZES, 4, at, 30, 13400))
    for sc in (scanner, hooks_scanner):
        def after(q0, q1):
            assert launches_per_class(sc) == {(3, 4): 1 if q1 - q0 < at else 2}
            if sc is hooks_scanner:
                got = sc.test_rowsweep_plan()
                assert got["forked"] and got["classes"][(3, 4)]["path"] == ("plain" if q1 - q0 < at else "segmented")
                assert q1 - q0 < at or got["classes"][(3, 4)]["chunk"] == at
        check_case(dcp, oracle32, sc, case, mode, [(0, below), (1, at), (0, at)], after)


def test_d2_single_stream(dcp, oracle32, hooks_scanner):
    """2048 profiles (copies of 32: 1 .. 8 nodes, twenty of 65 .. 128, the four of D1; tables expanded on the device) x
    2048 queries of 1 .. 6 nt (copies of 64) = 2^22 pairs: the launches stay on one stream, the {3, 4} class is
    segmented by the shipped rule, class 1 runs its one-profile kernels (2048 >= 96 queries), class 0 K profiles per
    wavefront; all 2^22 pairs in bits and the hit list.  Then 2047 queries of the same batch (forked): equal bits on
    the common rows."""
    sc = hooks_scanner
    case = the_case("D2", lambda: copies_case(dcp, "D2", pr.D2_SOURCES, pr.D2_NPROF, pr.D2_NQ, 6, 13500, on_host=False))
    assert len(case.profiles) * len(case.seqs) == 1 << 22

    def after(q0, q1):
        plan = sc.test_rowsweep_plan()
        assert plan["forked"] == (q1 - q0 < pr.D2_NQ)
        cl = plan["classes"]
        assert set(cl) == {(1, 1), (2, 1), (3, 4)}
        assert cl[(1, 1)]["path"] == "mp" and cl[(2, 1)]["path"] == "plain" and cl[(3, 4)]["path"] == "segmented"
        assert launches_per_class(sc) == {(1, 1): 1, (2, 1): 1, (3, 4): 2}
    for mode in MODES2:
        t0 = time.time()
        n = pr.D2_NQ
        out = check_case(dcp, oracle32, sc, case, mode, [(0, n), (0, n - 1)], after)
        assert np.array_equal(u32(out[(0, n)][0][:n - 1]), u32(out[(0, n - 1)][0]))
        assert np.array_equal(u32(out[(0, n)][1][:n - 1]), u32(out[(0, n - 1)][1]))
        print("D2 %s: %.1f s" % (mode_id(mode), time.time() - t0))


# ---- C: segments and chunks, forced on -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pr.C_MODES, ids=mode_id)
def test_c_segments_and_chunks(dcp, oracle32, hooks_scanner, mode):
    """Every multi-wavefront class at both ends, 2500 and 3072 nodes (one lane width, five and six segments), a
    delete-heavy and a flagged profile against 23 queries of 1 .. 120 nt and one-, back-to-back two- and spaced
    two-copy queries of the 513- (two segments) and the 1025-node (three) profile, the segmented sweep forced on, with
    column budgets computed from plan_segsweep's formula for chunks of 1, 3, 4, 5, nq - 1, nq and nq + 5 queries in the
    classes of two profiles (the class of three gets two thirds, the class of four half of that: at 1 none, and the hook
    must say it ran the exact kernel).  Every budget scans the whole batch and two ranges, one starting inside a chunk
    of the whole batch's scan.  A segmented class is two launches; its chunk is the formula's.  The pairs its last segment
    handed to the exact kernel (seg_redo: dcp_gpu_last_scan_redo_pairs does not count them, the hook does): in a uni-hit
    scan the flagged profile's only; with E -> B free AND N -> B closed (eb_only) every pair in which E is ever finite,
    i. e. all but the epsilon-0 profile's with queries of 1 and 2 nt and one that begins with TAA.  (With E -> B free alone -- eb_free, log1 -- the
    swept B(j) = N(j) + NB is NOT wrong for every pair: E(j) of a random query stays below N(j) + NB against a large
    profile, whose entry costs about log M; measured 12 of 58 pairs of the {4, 4} class re-scored, all bits right.
    There the count is only bounded.)  The same ranges with the segmented sweep forced off give the same bits and hit
    array."""
    case = the_case("C", lambda: Case("C", *pr.c_case(dcp, oracle32)[:2]))
    sc = hooks_scanner
    lens = [len(s) for s in case.seqs]
    counts = pr.c_class_counts()
    eps0_class = pr.class_of(next(pr.size_of(m) for m in pr.C_SIZES if isinstance(m, tuple) and m[1] == "eps0"))
    state = {}

    def after(q0, q1):
        nq = q1 - q0
        plan = sc.test_rowsweep_plan()
        nl = launches_per_class(sc)
        assert plan["forked"] and set(plan["classes"]) == set(counts)
        for k, (np_k, nflag) in counts.items():
            got, chunk = plan["classes"][k], state["chunks"][k]
            if chunk == 0:
                assert (got["path"], got["stage"], got["waves"]) == ("plain", 0, 1) and nl[k] == 1, (k, got)
                continue
            assert got["path"] == "segmented" and got["chunk"] == chunk and nl[k] == 2, (k, got, chunk, nl[k])
            if mode == "eb_only":
                # B(j) = N(j) + NB = -inf is wrong wherever E(j) is finite: at row 1 for a profile with frame shifts, at
                # row 3 for the one of epsilon 0 unless the query's first codon is missing or a stop codon
                never = sum(pr.e_never_finite_eps0(s) for s in case.seqs[q0:q1]) if k == eps0_class else 0
                assert got["seg_redo"] == np_k * nq - never, (k, got, never)
            elif mode in ((False, False), (False, True)):
                assert got["seg_redo"] == nflag * nq, (k, got)  # no E -> B, no J: only the flagged profile's pairs
            else:
                assert nflag * nq <= got["seg_redo"] <= np_k * nq, (k, got)
    ranges = pr.c_ranges(len(lens))
    try:
        sc.test_set_rowsweep_variant(-1, SEG_OFF)
        state["chunks"] = {k: 0 for k in counts}
        off = check_case(dcp, oracle32, sc, case, mode, ranges, after)
        sc.test_set_rowsweep_variant(-1, SEG_ON)
        for target in pr.C_CHUNKS:
            for q0, q1 in ranges:
                sub = lens[q0:q1]
                t = {"nq-1": len(sub) - 1, "nq": len(sub), "more": len(sub) + 5}.get(target, target)
                budget = pr.c_budget(t, sub)
                state["chunks"] = pr.c_expected_chunks(budget, sub)
                assert state["chunks"][(4, 4)] == min(t, len(sub))
                sc.test_set_seg_col_bytes(budget)
                on = check_case(dcp, oracle32, sc, case, mode, [(q0, q1)], after)[(q0, q1)]
                assert np.array_equal(u32(on[0]), u32(off[(q0, q1)][0])) and np.array_equal(u32(on[1]), u32(off[(q0, q1)][1]))
                assert np.array_equal(on[2], off[(q0, q1)][2])
    finally:
        sc.test_set_rowsweep_variant(-1, 0)
        sc.test_set_seg_col_bytes(0)
