"""The row sweeps' pair mode with more listed pairs than the grid holds (runs on a real MI355X).

viterbi_rowsweep_kernel<R, W, 0, false> with a.pairs set and viterbi64_kernel<R, false, true> score a list of
{query, profile}: the lists dcp_gpu_scan_pairs is given, the redo lists behind the query-lane kernels, seg_redo behind
the segmented sweep.  A block (float) or wavefront (double) takes a SECOND task only when the list is longer than the
launch; every case here makes one that long and asserts, from the test-hooks build's read-only
dcp_gpu_test_last_pair_launches (Scanner.test_pair_launches), that it was: trips = ceil(capacity / (units x tasks per
block)) >= 2.  Every list length is derived from the device's CU count (the driver's num_cus) by the rules
test_pair_mode_premises restates; the lists come from its deterministic builder.

Everything is compared in bits with the oracle's recursion in the DB's precision on the device's own tables
(orc_dp_tables: test_rowsweep_edge_premises.oracle_scores; Tables64 with oracle64.dp_tables), computed once per distinct
pair; hit lists as multisets of (seq_idx, profile_idx, null bits, alt bits) -- a pair listed m times comes back m times.

edge (dcp_kernels.hip / dcp_f64.hip)                                length derived from (dcp_gpu.hip)            reached by
  task loop `task += nblk * TASKS_PER_BLOCK` past its first trip;   dcp_gpu_scan_pairs: `g = min((count[k] + tpb    A: per class n = T - 1, T, T + 1,
  the XCD map vblk over a list longer than the grid                  - 1) / tpb, 8 * num_cus)`, T = tpb x 8 x CUs    2 T + 3 (1, 1, 2, 3 trips) and 1 .. 9
  W > 1: __syncthreads and the xc->flag reset between two tasks     the same line, tpb = 1                        A, B, C, D in the multi-wavefront classes
  W == 1: four wavefronts of a block with different trip counts     the same line, tpb = 4                        A at T + 1, 2 T + 3 (wavefronts 0 .. 2)
  long query -> 1-nt query -> long query, another profile of the    the builder: `stride` = blocks x tpb apart    A (asserted on the lists by the premises)
  class: fresh dcp_prof_meta, transitions, lane_off
  `min(*a.npairs, a.pair_cap)` with the counter past the capacity   launch_qlane_scan: `cap = min(pairs,           D: capacity n + 1, n, n - 1, T + 1, 1
  and the repeat scan                                                cap_limit)`, `redo_grid[k]`
  redo lists of the three float query-lane kernels                  launch_qlane_scan: `redo_grid[k]`             B: every class past its T, 2 kernels + w3
  seg_redo                                                          launch_segsweep_class: `g = min(ntasks, 8 *   C: 3 profiles x (8 CUs / 3 + 1) queries
                                                                     num_cus)`
  `pair += nw` in viterbi64_kernel<R, false, true>; a wavefront's   f64_seg_columns: `seg_waves = min(npairs, 2^27  A64: n = seg_waves - 1 .. 2 seg_waves + 3,
  column `a.col + gw * col_stride` reused by another pair            / col_stride)`                                 the 29 800-nt query at position 0
  kernel 4's redo launches                                          scan64: `waves = min(g == 3 ? seg_waves :      B64: > 4 096 pairs in all four groups;
                                                                     4096, min(redo_cap[g], 4096))`                 D64: the capacities of D on group 3
"""
import time

import numpy as np
import pytest
import torch  # before the product's library: both bring a HIP runtime, and torch must see the device too

import test_pair_mode_premises as pm
import test_rowsweep_edge_premises as pr
import test_rowsweep_edges as tre
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_f64_bits import Tables64, u64
from test_f64_edges import make_profiles as make_profiles64

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
u32 = tre.u32


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


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


@pytest.fixture(scope="module")
def hooks_scanner64(dcp):
    s = dcp.Scanner(0, lib=dcp.load_testhooks())
    yield s
    s.close()


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def rows(q, p, nb, ab):
    """the multiset of records as a sorted [n, 4] array of uint64"""
    a = np.stack([np.asarray(q, np.uint64), np.asarray(p, np.uint64), np.asarray(nb, np.uint64), np.asarray(ab, np.uint64)], axis=1)
    return a[np.lexsort(a.T[::-1])] if len(a) else a.reshape(0, 4)


def hit_rows(h, bits):
    return rows(h["seq_idx"], h["profile_idx"], bits(h["null_loglik"]), bits(h["alt_loglik"]))


def listed_rows(pairs, on, oa, bits, thr):
    """the reference's filter over the LIST: a listed pair as often as it is listed, iff its LRT is finite and not
    below thr (in the DB's precision)"""
    q, p = np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64)
    n, a = on[q, p], oa[q, p]
    with np.errstate(invalid="ignore", over="ignore"):
        lrt = n.dtype.type(-2) * (n - a)
        keep = np.isfinite(lrt) & ~(lrt < n.dtype.type(thr))
    return rows(q[keep], p[keep], bits(n[keep]), bits(a[keep])), int(keep.sum())


def assert_rows(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
        raise AssertionError("%s: %d records, %d wanted; first in one list only: %r (and by count: %r)" % (
            what, len(got), len(want), sorted(g ^ w)[:3], len(got) - len(want)))


def pair_accounting(profiles, seqs, pairs):
    M = np.array([profiles[p].core_size for _, p in pairs], np.int64)
    L = np.array([len(seqs[q]) for q, _ in pairs], np.int64)
    return int((M * L).sum()), int((20 * M * L + 32 * (M + 1) + L + 8).sum())


def float_case(dcp, oracle32, sc, key, make):
    """the Case (test_rowsweep_edges) of a key, resident on sc with fresh length-derived transitions"""
    case = memo(key, lambda: tre.Case(key, *make()))
    tre.upload(dcp, sc, case)
    sc.upload_seqs(case.seqs)
    return case


def float_scores(dcp, oracle32, case, mode):
    if mode not in case.scores:
        xt = pr.mode_xtrans(dcp, case.seqs, mode)
        case.scores[mode] = pr.oracle_scores(dcp, oracle32, case.profiles, case.tables, case.seqs, xt)
    return case.scores[mode]


# ---- A: scan_pairs over every size class ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", pm.A_N)
@pytest.mark.parametrize("lib", ["shipped", "hooks"])
def test_a_scan_pairs_past_the_grid(dcp, oracle32, scanner, hooks_scanner, lib, name):
    """All 14 size classes in one call, per class n = `name` listed pairs (T = tasks per block x 8 x CUs of the class):
    hits at -inf are the listed pairs with the oracle's bits and their multiplicity, at threshold 10 the oracle's
    filter over the list; the accounting of a pair scan; and from the hook 1 trip up to T, 2 at T + 1, 3 at 2 T + 3.
    Multi-hit; uni-hit and HMMER3-compatible too at T + 1."""
    t0 = time.time()
    cus = cu_count()
    sc = scanner if lib == "shipped" else hooks_scanner
    case = float_case(dcp, oracle32, sc, "pair/A", lambda: pm.a_case(dcp))
    per, whole = pm.a_lists(name, cus)
    sq, pp = [q for q, _ in whole], [p for _, p in whole]
    cells, nbytes = pair_accounting(case.profiles, case.seqs, whole)
    for mode in (pm.A_MODES if name == "T+1" else pm.A_MODES[:1]):
        what = "A %s %s %s" % (name, lib, tre.mode_id(mode))
        on, oa = float_scores(dcp, oracle32, case, mode)
        want, nwant = listed_rows(whole, on, oa, u32, NEG_INF)
        assert nwant == len(whole)  # the premise: every listed pair is finite
        sc.scan_pairs(sq, pp, mode[0], mode[1], NEG_INF)
        assert_rows(hit_rows(sc.hits(), u32), want, what)
        assert sc.cells == cells and sc.algorithmic_bytes == nbytes
        assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP and sc.last_scan_redo_pairs == 0
        assert sc.last_scan_launches == len(pm.CLASSES)
        infos = sc.launch_infos()
        assert len(infos) == len(pm.CLASSES) and sum(i["cells"] for i in infos) == cells
        assert sorted((i["R"], i["W"]) for i in infos) == sorted(pm.CLASSES)
        if lib == "hooks":
            got = sc.test_pair_launches()
            assert [(l["kind"], l["precision"]) for l in got] == [("scan_pairs", 32)] * len(pm.CLASSES)
            assert [l["cls"] for l in got] == pm.CLASSES
            for l in got:
                R, W = l["cls"]
                T, n = pm.T_of(W, cus), len(per[(R, W)])
                assert (l["cap"], l["tpb"], l["units"]) == (n, pm.tpb_of(W), pm.float_blocks(n, W, cus)), (what, l)
                want_trips = {"T+1": 2, "2T+3": 3}.get(name, 1)
                assert pm.trips(l["cap"], l["units"], l["tpb"]) == want_trips and (n > T) == (want_trips > 1), (what, l)
        sc.scan_pairs(sq, pp, mode[0], mode[1], 10.0)
        sel, nsel = listed_rows(whole, on, oa, u32, 10.0)
        assert_rows(hit_rows(sc.hits(), u32), sel, what + " threshold 10")
        assert len(whole) < 200 or 0 < nsel < len(whole)
    print("A %s %s: %d pairs, %.1f s" % (name, lib, len(whole), time.time() - t0))


# ---- B: the query-lane kernels' redo lists -------------------------------------------------------------------------
def check_qlane_scan(dcp, oracle32, sc, case, kernel, what, sync=True):
    """a multi-hit scan of the whole batch by `kernel` with dense scores at the median threshold: null, alt in bits,
    the hit list the filter's, every hit once.  sync=False: the caller looks at the hook before anything completes
    the scan."""
    on, oa = float_scores(dcp, oracle32, case, (True, False))
    assert not np.isnan(on).any() and not np.isnan(oa).any()
    nq = len(case.seqs)
    thr, hit, nfin = pr.median_filter(on, oa, 0, nq)
    sc.scan(True, False, float(thr), keep_scores=True, kernel=kernel, sync=sync)

    def finish():
        gn, ga = sc.scores()
        got = hit_rows(sc.hits(), u32)
        wq, wp = np.nonzero(hit)
        bad = np.argwhere((u32(gn) != u32(on)) | (u32(ga) != u32(oa)))
        assert len(bad) == 0, "%s: %d of %d pairs differ (%d hit records, %d wanted); first (query, profile) %r: device %r %r, oracle %r %r" % (
            what, len(bad), gn.size, len(got), len(wq), tuple(bad[0]), gn[tuple(bad[0])], ga[tuple(bad[0])], on[tuple(bad[0])], oa[tuple(bad[0])])
        assert_rows(got, rows(wq, wp, u32(on[wq, wp]), u32(oa[wq, wp])), what)
        assert 0 < len(wq) < gn.size
    if sync:
        finish()
    return finish


def class_pairs(case):
    out = {}
    for p in case.profiles:
        k = pr.class_of(p.core_size)
        out[k] = out.get(k, 0) + len(case.seqs)
    return out


def assert_redo_launches(sc, case, cus, what):
    """one redo launch per class, its capacity all the class's pairs, its grid the driver's rule; two trips or more"""
    got = sc.test_pair_launches()
    want = class_pairs(case)
    assert [(l["kind"], l["precision"]) for l in got] == [("qlane_redo", 32)] * len(want), (what, got)
    assert {l["cls"]: l["cap"] for l in got} == want, (what, got)
    for l in got:
        W = l["cls"][1]
        assert (l["tpb"], l["units"]) == (pm.tpb_of(W), pm.float_blocks(l["cap"], W, cus)), (what, l)
        assert l["cap"] > pm.T_of(W, cus) and pm.trips(l["cap"], l["units"], l["tpb"]) >= 2, (what, l)


@pytest.mark.parametrize("kernel", ["qlane", "qlane2"])
def test_b_redo_lists_past_the_grid(dcp, oracle32, hooks_scanner, kernel):
    """Flagged profiles only (positive MD / DD: every pair leaves the query-lane kernel through its class's redo list)
    in the classes (1,1), (8,1) and (3,4), against the fewest queries of 1 .. 40 nt that take all three lists past T."""
    t0 = time.time()
    cus, sc = cu_count(), hooks_scanner
    case = float_case(dcp, oracle32, sc, "pair/B", lambda: pm.b_case(dcp, cus))
    assert len(case.seqs) == pm.b_nq(cus)
    K = {"qlane": dcp.KERNEL_QLANE, "qlane2": dcp.KERNEL_QLANE2}[kernel]
    check_qlane_scan(dcp, oracle32, sc, case, K, "B " + kernel)
    assert sc.last_scan_kernel == K
    assert sc.last_scan_redo_pairs == len(case.seqs) * len(case.profiles)  # the premise: every pair is redone
    assert_redo_launches(sc, case, cus, "B " + kernel)
    print("B %s: %d pairs, %.1f s" % (kernel, len(case.seqs) * len(case.profiles), time.time() - t0))


def test_b_three_wavefront_kernel_s_redo_list(dcp, oracle32, hooks_scanner):
    """64 queries (KERNEL_QLANE then runs its three-wavefront variant) against T / 64 + 1 flagged profiles of 3 .. 8
    nodes: class (1,1)'s list passes T."""
    t0 = time.time()
    cus, sc = cu_count(), hooks_scanner
    case = float_case(dcp, oracle32, sc, "pair/B3", lambda: pm.b_w3_case(dcp, cus))
    assert len(case.seqs) == 64 and len(case.profiles) * 64 > pm.T_of(1, cus)
    check_qlane_scan(dcp, oracle32, sc, case, dcp.KERNEL_QLANE, "B w3")
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE
    assert sc.last_scan_redo_pairs == 64 * len(case.profiles)
    assert_redo_launches(sc, case, cus, "B w3")
    print("B w3: %d pairs, %.1f s" % (64 * len(case.profiles), time.time() - t0))


# ---- C: seg_redo ---------------------------------------------------------------------------------------------------
def test_c_seg_redo_past_the_grid(dcp, oracle32, hooks_scanner):
    """Three profiles of the (3,4) class against 8 CUs / 3 + 1 queries, the segmented sweep forced on, E -> B free and
    N -> B closed: every pair in which E is ever finite leaves through seg_redo (test_rowsweep_edges' "eb_only"), more
    than the 8 x CUs blocks of the exact kernel behind it.  The comparison is test_rowsweep_edges.check_case."""
    t0 = time.time()
    cus, sc = cu_count(), hooks_scanner
    case = memo("pair/C", lambda: tre.Case("pair/C", *pm.c_case(dcp, cus)))
    nq, npf = len(case.seqs), len(case.profiles)
    assert nq * npf > 8 * cus

    def after(q0, q1):
        plan = sc.test_rowsweep_plan()
        assert set(plan["classes"]) == {(3, 4)} and plan["classes"][(3, 4)]["path"] == "segmented"
        redo = plan["classes"][(3, 4)]["seg_redo"]
        assert redo == pm.c_seg_redo(case.seqs) and redo > 8 * cus  # all pairs but the epsilon-0 profile's without E
        got = sc.test_pair_launches()
        assert len(got) == 1 and (got[0]["kind"], got[0]["precision"], got[0]["cls"]) == ("seg_redo", 32, (3, 4)), got
        l = got[0]
        assert (l["cap"], l["tpb"], l["units"]) == (nq * npf, 1, pm.seg_redo_blocks(nq * npf, cus)), l
        assert l["units"] == 8 * cus and pm.trips(redo, l["units"]) == 2  # blocks took two tasks
    try:
        sc.test_set_rowsweep_variant(-1, tre.SEG_ON)
        tre.check_case(dcp, oracle32, sc, case, "eb_only", [(0, nq)], after)
    finally:
        sc.test_set_rowsweep_variant(-1, 0)
    print("C: %d pairs, %.1f s" % (nq * npf, time.time() - t0))


# ---- D: the redo lists' capacity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["qlane", "qlane2"])
def test_d_redo_capacity(dcp, oracle32, hooks_scanner, kernel):
    """The (3,4) class of B alone with n > T redo pairs, the list's capacity n + 1, n, n - 1, T + 1 and 1.  A list that
    holds all pairs: no repeat, n pairs redone.  A shorter one: its launch runs over min(counter, capacity) pairs --
    two trips at T + 1 -- and the scan is repeated with the row sweep: bits, every hit once (the truncated list's run
    appended records before the repeat zeroed the counter), and 0 redo pairs reported (finish_scan: "the float row
    sweep's does the same, and there 0 is what is reported")."""
    t0 = time.time()
    cus, sc = cu_count(), hooks_scanner
    case = float_case(dcp, oracle32, sc, "pair/D", lambda: pm.d_case(dcp, cus))
    n, T = len(case.seqs) * len(case.profiles), pm.T_of(4, cus)
    assert n > T and {pr.class_of(p.core_size) for p in case.profiles} == {(3, 4)}
    K = {"qlane": dcp.KERNEL_QLANE, "qlane2": dcp.KERNEL_QLANE2}[kernel]
    try:
        for c in dict.fromkeys((n + 1, n, n - 1, T + 1, 1)):
            what = "D %s capacity %d of %d" % (kernel, c, n)
            sc.test_set_redo_cap(c)
            finish = check_qlane_scan(dcp, oracle32, sc, case, K, what, sync=False)
            got = sc.test_pair_launches()  # before anything looks at the counters: the launches of the query-lane scan
            cap = min(n, c)
            assert len(got) == 1 and (got[0]["kind"], got[0]["cls"], got[0]["cap"]) == ("qlane_redo", (3, 4), cap), (what, got)
            assert got[0]["units"] == pm.float_blocks(cap, 4, cus) and got[0]["tpb"] == 1, (what, got)
            assert pm.trips(cap, got[0]["units"]) == (2 if cap > T else 1), (what, got)
            sc.sync()
            if c >= n:
                assert sc.last_scan_kernel == K and sc.last_scan_redo_pairs == n, what
                assert len(sc.test_pair_launches()) == 1
            else:
                assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP and sc.last_scan_redo_pairs == 0, what
                assert sc.test_pair_launches() == []  # the repeat is a dense row sweep
            finish()
    finally:
        sc.test_set_redo_cap(0)
    print("D %s: %d pairs x 5 capacities, %.1f s" % (kernel, n, time.time() - t0))


# ---- double --------------------------------------------------------------------------------------------------------
def oracle64_dense(oracle64, tabs, seqs, xt, pairs):
    """null, alt [nq, nprof] (NaN where not asked): orc_dp_tables in double on the device's tables over the distinct
    (query bytes, profile) of `pairs`; xt: [nq, 13]"""
    on = np.full((len(seqs), len(tabs.t)), np.nan)
    oa = on.copy()
    done = {}
    for q, p in sorted(set(pairs)):
        key = (bytes(seqs[q]), p)
        if key not in done:
            t8, em, ei, en = tabs.t[p]
            rc, nl, al = oracle64.dp_tables(t8, em, ei, en, xt[q], bytes(seqs[q]))
            assert rc == 0
            done[key] = (nl, al)
        on[q, p], oa[q, p] = done[key]
    return on, oa


@pytest.mark.parametrize("name", pm.A64_N)
def test_a64_scan_pairs_past_seg_waves(dcp, oracle64, hooks_scanner64, name):
    """scan_pairs on a double DB: the segmented group's list (257, 300, 513 nodes) as long as seg_waves - 1, seg_waves,
    seg_waves + 1 and 2 seg_waves + 3, seg_waves about 900 for the 29 800-nt query listed once at position 0 -- its
    wavefront's boundary column then serves short pairs; the other groups' lists of 1 .. 9.  Bits, multiset, accounting,
    and the hook's wavefront count."""
    t0 = time.time()
    sc = hooks_scanner64
    profs, seqs, tabs = memo("pair/A64", lambda: a64_world(dcp, oracle64, sc))
    if _memo.get("resident64") != "A64":
        sc.upload_db(profs)
        _memo["resident64"] = "A64"
    sc.upload_seqs(seqs)
    per, whole = pm.a64_lists(name)
    xt = np.stack([dcp.xtrans64(len(s), True, False) for s in seqs])
    on, oa = memo("pair/A64/scores", lambda: oracle64_dense(oracle64, tabs, seqs, xt, pm.a64_lists("2sw+3")[1] +
                                                           [p for n in pm.A64_N for p in pm.a64_lists(n)[1][:40]]))
    sw = pm.seg_waves(pm.A64_LMAX, 10 ** 9)
    n3 = len(per[3])
    sq, pp = [q for q, _ in whole], [p for _, p in whole]
    want, nwant = listed_rows(whole, on, oa, u64, NEG_INF)
    assert nwant == len(whole)
    sc.scan_pairs(sq, pp, True, False, NEG_INF)
    assert_rows(hit_rows(sc.hits(), u64), want, "A64 " + name)
    cells, nbytes = pair_accounting(profs, seqs, whole)
    assert sc.cells == cells and sc.algorithmic_bytes == nbytes
    assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP and sc.last_scan_redo_pairs == 0 and sc.last_scan_launches == 4
    got = sc.test_pair_launches()
    assert [(l["kind"], l["precision"], l["group"], l["tpb"]) for l in got] == [("scan_pairs", 64, g, 1) for g in range(4)]
    assert [l["cap"] for l in got] == [len(per[g]) for g in range(4)]
    assert [l["units"] for l in got] == [pm.f64_pair_waves(g, len(per[g]), pm.A64_LMAX) for g in range(4)]
    assert got[3]["units"] == min(n3, sw) and pm.trips(n3, got[3]["units"]) == {"sw+1": 2, "2sw+3": 3}.get(name, 1)
    # the filter at the median LRT of the listed pairs (random queries: none reaches 10)
    thr = float(np.median(-2 * (on - oa)[np.array(sq), np.array(pp)]))
    sc.scan_pairs(sq, pp, True, False, thr)
    sel, nsel = listed_rows(whole, on, oa, u64, thr)
    assert_rows(hit_rows(sc.hits(), u64), sel, "A64 %s threshold %r" % (name, thr))
    assert 0 < nsel < len(whole)
    print("A64 %s: %d pairs, %.1f s" % (name, len(whole), time.time() - t0))


def a64_world(dcp, oracle64, sc):
    profs, _ = make_profiles64(dcp, oracle64, pm.a64_params(), [ENTRY_DIST_OCCUPANCY] * len(pm.A64_SIZES))
    seqs = pm.a64_queries()
    sc.upload_db(profs)
    _memo["resident64"] = "A64"
    return profs, seqs, Tables64(sc, profs)


def b64_world(dcp, oracle64, sc, key, sizes):
    """profiles of `sizes` resident on sc, b64_nq() queries of 1 .. 40 nt with E -> B, J -> B free and N -> B closed;
    the oracle's dense scores on the device's tables (distinct queries once)"""
    def make():
        profs, _ = make_profiles64(dcp, oracle64, pm.b64_params(sizes), [ENTRY_DIST_OCCUPANCY] * len(sizes))
        seqs = pm.b64_queries(pm.b64_nq())
        sc.upload_db(profs)
        tabs = Tables64(sc, profs)
        xt = pm.eb_only64(dcp, seqs)
        on, oa = oracle64_dense(oracle64, tabs, seqs, xt, [(q, p) for q in range(len(seqs)) for p in range(len(profs))])
        return profs, seqs, xt, on, oa
    profs, seqs, xt, on, oa = memo(key, make)
    if _memo.get("resident64") != key:
        sc.upload_db(profs)
        _memo["resident64"] = key
    sc.upload_seqs(seqs)
    sc.set_xtrans64(xt)
    return profs, seqs, on, oa


def check_dense64(sc, on, oa, thr, what):
    gn, ga = sc.scores()
    got = hit_rows(sc.hits(), u64)
    with np.errstate(invalid="ignore"):
        lrt = -2 * (on - oa)
        hit = np.isfinite(lrt) & ~(lrt < thr)
    wq, wp = np.nonzero(hit)
    bad = np.argwhere((u64(gn) != u64(on)) | (u64(ga) != u64(oa)))
    assert len(bad) == 0, "%s: %d of %d pairs differ (%d hit records, %d wanted); first %r: device %r %r, oracle %r %r" % (
        what, len(bad), gn.size, len(got), len(wq), tuple(bad[0]), gn[tuple(bad[0])], ga[tuple(bad[0])], on[tuple(bad[0])], oa[tuple(bad[0])])
    assert_rows(got, rows(wq, wp, u64(on[wq, wp]), u64(oa[wq, wp])), what)  # every hit once
    assert 0 < len(wq) < on.size
    return gn, ga


def median_lrt64(on, oa):
    with np.errstate(invalid="ignore"):
        lrt = -2 * (on - oa)
    return float(np.median(lrt[np.isfinite(lrt)]))


def test_b64_kernel4_redo_lists_past_4096(dcp, oracle64, hooks_scanner64):
    """Kernel 4 on three profiles per launch group (64, 128, 256 and 257 .. 300 nodes) x 4096 / 3 + 1 queries with
    E -> B, J -> B free and N -> B closed: every pair leaves through its group's redo list, each longer than the 4 096
    wavefronts of its launch.  Dense scores in bits against the oracle and against kernel 1."""
    t0 = time.time()
    sc = hooks_scanner64
    profs, seqs, on, oa = b64_world(dcp, oracle64, sc, "pair/B64", pm.B64_SIZES)
    nq = len(seqs)
    thr = median_lrt64(on, oa)
    sc.scan(True, False, thr, keep_scores=True, kernel=dcp.KERNEL_QLANE64)
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE64
    assert sc.last_scan_redo_pairs == nq * len(profs)  # the premise: every pair is redone
    got = sc.test_pair_launches()
    assert [(l["kind"], l["precision"], l["group"], l["tpb"]) for l in got] == [("qlane_redo", 64, g, 1) for g in range(4)]
    for l in got:
        assert l["cap"] == 3 * nq > pm.F64_REDO_WAVES == l["units"] and pm.trips(l["cap"], l["units"]) >= 2, l
        assert l["units"] == pm.f64_redo_waves(l["group"], l["cap"], nq, 3, max(len(s) for s in seqs))
    gn4, ga4 = check_dense64(sc, on, oa, thr, "B64 kernel 4")
    sc.scan(True, False, thr, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    gn1, ga1 = check_dense64(sc, on, oa, thr, "B64 kernel 1")
    assert sc.test_pair_launches() == []
    assert np.array_equal(u64(gn4), u64(gn1)) and np.array_equal(u64(ga4), u64(ga1))
    print("B64: %d pairs, %.1f s" % (nq * len(profs), time.time() - t0))


def test_d64_redo_capacity(dcp, oracle64, hooks_scanner64):
    """Group 3 of B64 alone, n = 3 x (4096 / 3 + 1) redo pairs, capacities n + 1, n, n - 1, 4 097 and 1.  Below n the
    scan is repeated with the row sweep; the redo pairs reported stay the figure the lists took (finish_scan: "what the
    lists took stays the figure reported"): the device counter, which counts on past the capacity -- n."""
    t0 = time.time()
    sc = hooks_scanner64
    profs, seqs, on, oa = b64_world(dcp, oracle64, sc, "pair/D64", pm.B64_SIZES[9:])
    nq = len(seqs)
    n, T = nq * len(profs), pm.F64_REDO_WAVES
    assert n > T and {pm.f64_group_of(p.core_size) for p in profs} == {3}
    thr = median_lrt64(on, oa)
    try:
        for c in dict.fromkeys((n + 1, n, n - 1, T + 1, 1)):
            what = "D64 capacity %d of %d" % (c, n)
            sc.test_set_redo_cap(c)
            sc.scan(True, False, thr, keep_scores=True, kernel=dcp.KERNEL_QLANE64, sync=False)
            got = sc.test_pair_launches()  # before anything looks at the counters
            cap = min(n, c)
            assert len(got) == 1 and (got[0]["kind"], got[0]["group"], got[0]["cap"]) == ("qlane_redo", 3, cap), (what, got)
            assert got[0]["units"] == pm.f64_redo_waves(3, cap, nq, 3, max(len(s) for s in seqs)) == min(cap, T), (what, got)
            assert pm.trips(cap, got[0]["units"]) == (2 if cap > T else 1), (what, got)
            sc.sync()
            assert sc.last_scan_kernel == (dcp.KERNEL_QLANE64 if c >= n else dcp.KERNEL_ROWSWEEP), what
            assert sc.last_scan_redo_pairs == n, what
            assert len(sc.test_pair_launches()) == (1 if c >= n else 0)
            check_dense64(sc, on, oa, thr, what)
    finally:
        sc.test_set_redo_cap(0)
    print("D64: %d pairs x 4 capacities, %.1f s" % (n, time.time() - t0))
