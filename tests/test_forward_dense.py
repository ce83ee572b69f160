"""The dense Forward scan, the exponential tail fit on the device and Forward E-values (runs on a real MI355X):
dcp_gpu_forward_dense / dcp_gpu_fetch_forward_scores (csrc/dcp_gpu.hip; the lists come from dense_pairs_kernel,
csrc/dcp_forward.hip), dcp_gpu_fit_exp_tail (exp_tail_fit_kernel, csrc/dcp_calib.hip), dcp_gpu_db_calibrate_forward,
dcp_scores_evalues.

Nothing here has a tolerance of its own.  A pair's sweep does not depend on what else is in a launch, so every entry of
the dense matrices is compared IN BITS with forward_pairs of the full q-major list -- the kernels, and whether they are
right, are tests/test_forward_pairs.py's and tests/test_forward_chain_edges.py's business.  The fit is compared with the
host twin on the same fetched columns: tau, k_eff, status and lambda in bits, mu within 2^-32 (|mu| + 1 / lambda),
tests/test_gumbel_fit.py's bound for a result behind one log and one division.

Profiles of 1, 63, 64, 65, 128, 129, 256, 257 and 513 nodes: every class of the kernels and each class edge; sequences of
1, 5, 6, 17 and 40 nt.  Rounds of 1, 7, P - 1, P + 1 and all but one pair cut the line of pairs inside classes and between
them; a delete-heavy and a severed 1100-node profile of tests/test_forward_chain_premises.py's world check that a wide
pair's work area survives a round boundary."""
import ctypes as C

import numpy as np
import pytest

import test_forward_chain_premises as pr
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, hit_fields, refused
from test_forward_chain_edges import index_of
from test_forward_pairs import FLAGS, NEG_INF, PRECISIONS, xtrans_of
from test_gpu_parity import pfam_like_params
from test_gumbel_fit import LANE_N, LANE_NPROF, REL, lane_profiles
from test_gumbel_tail import same_bits, tail_counts
from test_seq_windows import PLANT_L, planted_world

DENSE_M = (1, 63, 64, 65, 128, 129, 256, 257, 513)
DENSE_L = (1, 5, 6, 17, 40)
_WORLD = {}


def dense_world(dcp, precision):
    """the nine profiles, an epsilon-0 profile of 70 nodes for a tenth, and the batch B"""
    if precision not in _WORLD:
        rng = np.random.default_rng(2300 + precision)
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
        profs = [dcp.ProteinProfile.from_params(*pfam_like_params(rng, M), cfg, f"DNS{M}", precision=precision) for M in DENSE_M]
        eps0 = dcp.ProteinProfile.sample(77, 70, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
        seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in DENSE_L]
        _WORLD[precision] = (profs, eps0, seqs)
    return _WORLD[precision]


def full_list(sc):
    """every pair, q-major: the dense layout"""
    n, P = sc.nseqs, sc.nprofiles
    return np.arange(n).repeat(P), np.tile(np.arange(P), n)


def pairs_as_matrices(sc, multi=True, h3=False):
    sq, pr_ = full_list(sc)
    nl, al = sc.forward_pairs(sq, pr_, multi, h3)
    return nl.reshape(sc.nseqs, sc.nprofiles), al.reshape(sc.nseqs, sc.nprofiles)


def same_matrices(got, want):
    return all(g.shape == w.shape and g.dtype == np.float64 and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def dense(sc, multi=True, h3=False):
    sc.forward_dense(multi, h3)
    return sc.forward_scores()


def host_exp_fits(dcp, null, alt, k):
    """the host twin on the columns of fetched matrices: (mu, lam, status, tau, k_eff) arrays"""
    with np.errstate(invalid="ignore"):  # -inf - -inf of an epsilon = 0 lane
        x = alt.astype(np.float64) - null.astype(np.float64)
    fits = [dcp.exp_tail_fit(x[:, p], k) for p in range(x.shape[1])]
    return (np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[2] for f in fits], np.uint8),
            np.array([f[3] for f in fits]), np.array([f[4] for f in fits], np.uint32))


def compare_exp_fits(got, want, where):
    """tau, k_eff, statuses and lambda in bits, NaN where not OK, mu within the bound: its maximum"""
    (gm, gl, gs, gt, gk), (wm, wl, ws, wt, wk) = got, want
    assert gs.dtype == np.uint8 and np.array_equal(gs, ws), (where, gs, ws)
    assert gk.dtype == np.uint32 and np.array_equal(gk, wk), (where, gk, wk)
    assert same_bits(gt, wt) and same_bits(gl, wl), (where, gt, wt, gl, wl)
    ok = ws == 0
    assert np.isnan(gm[~ok]).all() and np.isnan(gl[~ok]).all(), where
    if not ok.any():
        return 0.0
    dm = np.abs(gm[ok] - wm[ok]) / (np.abs(wm[ok]) + 1.0 / wl[ok])
    assert (gl[ok] > 0).all() and dm.max() <= REL, (where, dm.max())
    return float(dm.max())


# ---- the dense scan ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dense_equals_the_pair_list(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    sc = dcp.Scanner(0)
    assert sc.forward_dense_kernel_ms() < 0
    refused(dcp, sc, sc.forward_dense)  # no DB
    sc.upload_db(profs + [eps0])
    refused(dcp, sc, sc.forward_dense)  # no batch
    sc.upload_seqs(seqs)
    refused(dcp, sc, sc.forward_scores)  # none computed yet
    refused(dcp, sc, lambda: sc.fit_exp_tail(2))
    assert sc.forward_dense_kernel_ms() < 0  # negative before the first launch
    seen = set()
    for multi, h3 in FLAGS:
        got = dense(sc, multi, h3)
        assert sc.forward_dense_kernel_ms() > 0
        want = pairs_as_matrices(sc, multi, h3)
        assert got[0].shape == (len(seqs), len(profs) + 1) and same_matrices(got, want), (precision, multi, h3)
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
        # the epsilon-0 profile: -inf twice where L mod 3 != 0
        for q, s in enumerate(seqs):
            if len(s) % 3:
                assert got[0][q, -1] == NEG_INF and got[1][q, -1] == NEG_INF
        assert np.isfinite(got[1][:, :-1]).sum() > got[1][:, :-1].size // 2
        seen.add(got[1].tobytes())
    assert len(seen) == len(FLAGS)  # the flags reach the sweeps
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounds_and_wavefront_caps_change_no_bit(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    P, B = len(profs), len(seqs)
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    base = dense(sc)
    assert same_matrices(base, pairs_as_matrices(sc))
    for npairs in (1, 7, P - 1, P + 1, B * P - 1):
        sc.test_set_dense_round(npairs)
        assert same_matrices(dense(sc), base), (precision, npairs)
    sc.test_set_dense_round(0)
    for cap in (1, 3):
        sc.test_set_forward_waves(cap)
        assert same_matrices(dense(sc), base), (precision, cap)
    sc.test_set_dense_round(7)  # both at once
    assert same_matrices(dense(sc), base)
    sc.test_set_forward_waves(0)
    sc.test_set_dense_round(0)

    # two wide profiles of the chain world in the same batch: their work areas across round boundaries
    specs = pr.world_specs()
    wide = [specs[index_of(specs, "delete", 1100)], specs[index_of(specs, "severed", 1100, 512)]]
    chain = [dcp.ProteinProfile.from_params(*pr.chain_params(fam, M, k), dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, eps),
                                            "%s%d_%s" % (fam, M, k), precision=precision) for fam, M, k, eps in wide]
    mine = profs[:4] + [chain[0]] + profs[4:] + [chain[1]]
    sc.upload_db(mine)
    refused(dcp, sc, sc.forward_scores)  # void with the DB
    sc.upload_seqs(pr.world_queries() + seqs)
    base = dense(sc)
    assert same_matrices(base, pairs_as_matrices(sc))
    at = [4, len(mine) - 1]
    assert np.isfinite(base[1][:, at]).any(axis=0).all() and (base[1][:, at[0]] != base[1][:, at[1]]).any()
    for npairs, cap in ((1, 0), (3, 0), (7, 1), (len(mine) + 1, 3), (2 * sc.nseqs - 1, 0), (2 * sc.nseqs - 1, 1)):
        sc.test_set_dense_round(npairs)
        sc.test_set_forward_waves(cap)
        assert same_matrices(dense(sc), base), (precision, npairs, cap)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_batches_and_explicit_transitions(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    rng = np.random.default_rng(5)
    longer = [rng.integers(0, 4, L, dtype=np.uint8) for L in (333, 100, 64, 17)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    # both strands
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()
    got = dense(sc)
    assert got[0].shape[0] == 2 * len(seqs) and same_matrices(got, pairs_as_matrices(sc))
    assert not np.array_equal(got[1][:len(seqs)], got[1][len(seqs):])
    # windows, then both strands of them
    sc.upload_seqs(longer)
    sc.cut_windows(64, 40)
    got = dense(sc, False, False)
    assert got[0].shape[0] == sc.nseqs > len(longer) and same_matrices(got, pairs_as_matrices(sc, False, False))
    sc.add_reverse_strand()
    assert same_matrices(dense(sc), pairs_as_matrices(sc))
    # regions
    sc.upload_seqs(longer)
    sc.cut_regions([0, 0, 1], [0, 100, 30], [333, 150, 64], [0, 1, 0])
    got = dense(sc)
    assert got[0].shape[0] == 3 and same_matrices(got, pairs_as_matrices(sc))
    # explicit transitions in the DB's precision: the flags are ignored, the scores move
    sc.upload_seqs(seqs)
    derived = dense(sc)
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    refused(dcp, sc, sc.forward_scores)  # void with the transitions
    got = dense(sc)
    assert same_matrices(got, pairs_as_matrices(sc)) and same_matrices(got, dense(sc, False, True))
    assert not np.array_equal(got[1], derived[1])
    # those of the other precision are refused, as forward_pairs refuses them
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, sc.forward_dense)
    refused(dcp, sc, sc.forward_scores)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lifetimes(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sq, pr_ = np.array([4, 3, 4, 2, 0]), np.array([8, 5, 0, 7, 3])

    def flat(x):
        """every array of a result, nested lists included, as bytes"""
        if isinstance(x, (tuple, list)):
            return [flat(v) for v in x]
        return np.ascontiguousarray(x).tobytes()

    # a scan and the pair-list calls before a dense scan ...
    sc.scan(True, False, NEG_INF, keep_scores=True)
    before = (flat(sc.scores()), hit_fields(sc.hits()), sc.cells, sc.last_scan_launches, sc.last_scan_kernel)
    assert len(before[1][0]) > 0
    calls = (lambda: sc.forward_pairs(sq, pr_), lambda: sc.posterior_pairs(sq, pr_), lambda: sc.mea_pairs(sq, pr_))
    lists = [flat(call()) for call in calls]
    kept = dense(sc, False, False)  # other flags than the scan's
    # ... and behind it
    assert (flat(sc.scores()), hit_fields(sc.hits()), sc.cells, sc.last_scan_launches, sc.last_scan_kernel) == before
    sc.fit_gumbel()  # the scan's dense scores still serve its fits
    assert [flat(call()) for call in calls] == lists
    # the matrices behind a scan and each pair-list call
    assert same_matrices(sc.forward_scores(), kept)
    sc.scan(True, False, 10.0, keep_scores=True)
    assert same_matrices(sc.forward_scores(), kept)
    sc.scan_pairs(sq, pr_)
    assert same_matrices(sc.forward_scores(), kept)
    for call in calls:
        call()
        assert same_matrices(sc.forward_scores(), kept)
    fit = sc.fit_exp_tail(3)
    assert same_matrices(sc.forward_scores(), kept)
    # void from the moment the DB or the batch is replaced, or the transitions change: a message, outputs untouched
    null, alt = np.full(kept[0].shape, 1.5), np.full(kept[0].shape, 2.5)
    out5 = [np.full(len(profs), 9.0), np.full(len(profs), 9.0), np.full(len(profs), 9, np.uint8), np.full(len(profs), 9.0),
            np.full(len(profs), 9, np.uint32)]

    def void(why):
        assert sc._lib.dcp_gpu_fetch_forward_scores(sc._c, null.ctypes.data, alt.ctypes.data) == dcp.RC_EINVAL, why
        assert "no dense Forward scores" in sc._lib.dcp_gpu_last_error(sc._c).decode(), why
        assert sc._lib.dcp_gpu_fit_exp_tail(sc._c, dcp.SCORES_FORWARD, 2, *[a.ctypes.data for a in out5]) == dcp.RC_EINVAL, why
        assert "no dense Forward scores" in sc._lib.dcp_gpu_last_error(sc._c).decode(), why
        assert (null == 1.5).all() and (alt == 2.5).all() and all((a == 9).all() for a in out5), why
        refused(dcp, sc, sc.forward_scores)
        refused(dcp, sc, lambda: sc.fit_exp_tail(2))

    changes = (("an upload", lambda: sc.upload_seqs(seqs)), ("a random batch", lambda: sc.random_seqs(5, 17, 3)),
               ("the reverse strand", sc.add_reverse_strand), ("windows", lambda: (sc.random_seqs(5, 17, 3), sc.forward_dense(), sc.cut_windows(8, 4))),
               ("regions", lambda: (sc.upload_seqs(seqs), sc.forward_dense(), sc.cut_regions([4, 3], [0, 2], [40, 9], [0, 1]))),
               ("explicit transitions", lambda: (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(
                   np.stack([xtrans_of(dcp, precision, 9, True, False)] * sc.nseqs))),
               ("a DB", lambda: sc.upload_db(profs[:3])))
    for why, change in changes:
        assert sc.forward_scores()[0].shape == (sc.nseqs, sc.nprofiles)  # valid until the change
        change()
        void(why)
        if sc.nprofiles == len(profs):
            sc.forward_dense()
    # null outputs, an unknown source, a tail count outside the batch
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.forward_dense(False, False)
    assert same_matrices(sc.forward_scores(), kept)
    for x, y in zip(sc.fit_exp_tail(3), fit):
        assert same_bits(x, y)
    assert sc._lib.dcp_gpu_fetch_forward_scores(sc._c, None, alt.ctypes.data) == dcp.RC_EINVAL
    assert sc._lib.dcp_gpu_fetch_forward_scores(sc._c, null.ctypes.data, None) == dcp.RC_EINVAL
    for i in range(5):
        args = [a.ctypes.data for a in out5]
        args[i] = None
        assert sc._lib.dcp_gpu_fit_exp_tail(sc._c, dcp.SCORES_FORWARD, 2, *args) == dcp.RC_EINVAL
        assert "null output" in sc._lib.dcp_gpu_last_error(sc._c).decode()
    for source, k in ((2, 2), (-1, 2), (dcp.SCORES_FORWARD, 1), (dcp.SCORES_FORWARD, len(seqs) + 1), (dcp.SCORES_FORWARD, 0)):
        assert sc._lib.dcp_gpu_fit_exp_tail(sc._c, source, k, *[a.ctypes.data for a in out5]) == dcp.RC_EINVAL
    assert all((a == 9).all() for a in out5)
    with pytest.raises(dcp.DcpError):
        sc.fit_exp_tail(2, source="viterbi")
    sc.close()


class DenseArgs(C.Structure):
    """struct dcp_fwd_dense_args (csrc/dcp_forward.h)"""
    _fields_ = [("seq_order", C.c_void_p), ("prof_order", C.c_void_p), ("class_first", C.c_uint32 * 5), ("nseqs", C.c_uint32),
                ("nprof", C.c_uint32), ("t0", C.c_uint32), ("n", C.c_uint32), ("pairs", C.c_void_p)]


def test_the_list_launcher_refuses_on_the_host(dcp):
    """CPU: what dcp_forward_dense_pairs_launch refuses, it refuses before it touches the device -- an outer product past
    32 bits, a round that reaches past the line's end, class bounds that are not a partition, nothing to write, a null
    pointer.  (The pointers are never followed on the host.)"""
    fn = dcp.lib.dcp_forward_dense_pairs_launch
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]

    def launch(nseqs, nprof, t0, n, first=None, ptrs=(8, 8, 8)):
        a = DenseArgs(ptrs[0], ptrs[1], (C.c_uint32 * 5)(*(first or (0, nprof, nprof, nprof, nprof))), nseqs, nprof, t0, n, ptrs[2])
        return fn(C.addressof(a), None)

    assert launch(65536, 65536, 0, 1) != 0  # 2^32 pairs
    assert launch(2 ** 32 - 1, 2, 0, 1) != 0
    assert launch(33038210, 130, 0, 1) != 0  # the size test_past_32_bits_is_refused makes resident
    assert launch(5, 9, 40, 6) != 0  # 46 > 45
    assert launch(5, 9, 45, 1) != 0
    assert launch(5, 9, 0, 0) != 0
    assert launch(0, 9, 0, 1) != 0 and launch(5, 0, 0, 1) != 0
    assert launch(5, 9, 0, 5, first=(0, 3, 2, 9, 9)) != 0 and launch(5, 9, 0, 5, first=(1, 3, 3, 9, 9)) != 0
    assert launch(5, 9, 0, 5, first=(0, 3, 3, 8, 8)) != 0
    for i in range(3):
        ptrs = [8, 8, 8]
        ptrs[i] = None
        assert launch(5, 9, 0, 5, ptrs=ptrs) != 0
    assert fn(None, None) != 0


@pytest.mark.gpu
def test_past_32_bits_is_refused(dcp):
    """130 profiles x 33 038 210 one-base sequences = 2^32 + 4: refused on the host, with a message, before anything runs"""
    sc = dcp.Scanner(0)
    sc.upload_db(lane_profiles(dcp, 32, 130))
    n = -(-2 ** 32 // 130)
    assert (n - 1) * 130 <= 2 ** 32 - 1 < n * 130
    sc.random_seqs(n, 1, 1)
    with pytest.raises(dcp.DcpError) as e:
        sc.forward_dense()
    assert e.value.rc == dcp.RC_EINVAL and "2^32" in str(e.value)
    assert sc.forward_dense_kernel_ms() < 0
    refused(dcp, sc, sc.forward_scores)
    sc.close()


# ---- the fit at the lane edges -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nprof", LANE_NPROF)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_fit_of_scan_scores_equals_the_host_twin(dcp, precision, nprof):
    sc = dcp.Scanner(0)
    assert sc.exp_tail_kernel_ms(0) < 0 and sc.exp_tail_kernel_ms(1) < 0
    sc.upload_db(lane_profiles(dcp, precision, nprof))
    worst = 0.0
    for n in LANE_N:
        sc.random_seqs(n, 100, 40 + n)
        sc.scan(True, False, 10.0)
        null, alt = sc.scores()
        assert null.dtype == (np.float64 if precision == 64 else np.float32)
        for k in tail_counts(n):
            gumbel = sc.fit_gumbel_tail(k)
            got = sc.fit_exp_tail(k, source="scan")
            assert (got[4] >= k).all() and (got[4] <= n).all()
            worst = max(worst, compare_exp_fits(got, host_exp_fits(dcp, null, alt, k), (precision, nprof, n, k)))
            assert same_bits(got[3], gumbel[3]) and np.array_equal(got[4], gumbel[4])  # one selection
            if k == n:
                ok = got[2] == dcp.FIT_OK
                assert same_bits(got[0][ok], got[3][ok])  # mu = tau = the minimum
    assert sc.exp_tail_kernel_ms(0) > 0 and sc.exp_tail_kernel_ms(1) > 0 and sc.exp_tail_kernel_ms(2) < 0
    # tied rows from duplicated sequences: k_eff > k
    a, b, c = (dcp.random_seq(11, q, 100) for q in range(3))
    sc.upload_seqs([a, c, b, a] + [dcp.random_seq(12, q, 100) for q in range(6)] + [a, b, c, a])
    sc.scan(True, False, 10.0)
    null, alt = sc.scores()
    x = alt.astype(np.float64) - null.astype(np.float64)
    n, widened, flat = len(x), 0, 0
    for k in range(2, n + 1):
        got = sc.fit_exp_tail(k, source="scan")
        tau = np.sort(x, axis=0)[n - k]
        assert np.array_equal(got[3], tau) and np.array_equal(got[4], (x >= tau).sum(axis=0))
        all_tied = (np.where(x >= tau, x, tau) == tau).all(axis=0)
        assert np.array_equal(got[2] == dcp.FIT_FLAT, all_tied) and (got[2][~all_tied] == dcp.FIT_OK).all()
        widened += int((got[4] > k).sum())
        flat += int(all_tied.sum())
        compare_exp_fits(got, host_exp_fits(dcp, null, alt, k), (precision, nprof, "tied", k))
    # (one profile may well have one of the six single sequences on top: its small tails then are neither tied nor flat)
    assert nprof == 1 or (widened > 0 and flat > 0)
    print("precision %d, %d profiles, scan scores: device vs host twin, lambda in bits, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % (precision, nprof, worst))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nprof", LANE_NPROF)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_fit_of_forward_scores_equals_the_host_twin(dcp, precision, nprof):
    """a random batch of 30 nt; one NONFINITE lane, an epsilon-0 profile (30 nt is a multiple of 3, yet a stop codon in
    frame leaves some sequence without a path: asserted), sits among OK ones"""
    profs = list(lane_profiles(dcp, precision, nprof))
    at = min(37, nprof - 1)
    zero = dcp.ProteinProfile.sample(999, 40, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    if nprof > 1:
        profs[at] = zero
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    worst = 0.0
    for n in LANE_N:
        sc.random_seqs(n, 30, 40 + n)
        null, alt = dense(sc)
        assert null.dtype == np.float64 and null.shape == (n, nprof)
        for k in tail_counts(n):
            got = sc.fit_exp_tail(k)
            worst = max(worst, compare_exp_fits(got, host_exp_fits(dcp, null, alt, k), (precision, nprof, n, k)))
            rest = np.arange(nprof) != at if nprof > 1 else np.ones(1, bool)
            assert (got[2][rest] != dcp.FIT_NONFINITE).all() and (got[4][rest] >= k).all()
            if nprof > 1 and n >= 64:
                assert not np.isfinite(alt[:, at]).all()
                assert got[2][at] == dcp.FIT_NONFINITE and np.isnan(got[3][at]) and got[4][at] == 0
                assert (got[2][rest] == dcp.FIT_OK).sum() >= nprof - 2
    print("precision %d, %d profiles, Forward scores: device vs host twin, lambda in bits, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % (precision, nprof, worst))
    sc.close()


# ---- the composed call ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_calibrate_forward_is_its_three_steps(dcp, precision):
    profs = lane_profiles(dcp, precision, 65)
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    n, L, seed, k, probs = 80, 45, 77, 20, (0.3, 0.2, 0.2, 0.3)
    got = a.calibrate_forward(n, L, seed, k, probs, multi_hits=False, hmmer3_compat=False)
    b.random_seqs(n, L, seed, probs)
    b.forward_dense(False, False)
    want = b.fit_exp_tail(k)
    assert len(got) == 5 and got[4].dtype == np.uint32
    for x, y in zip(got, want):
        assert same_bits(x, y), precision
    assert (got[2] == dcp.FIT_OK).sum() >= 0.9 * len(profs) and (got[4] >= k).all()
    # what it leaves: the random batch and the matrices
    assert (a.nseqs, a.strands, a.windows) == (n, 1, None)
    ids, cap, ln = np.zeros(L, np.uint8), L, C.c_uint(0)
    assert a._lib.dcp_gpu_seqs_fetch(a._c, 0, ids.ctypes.data, cap, C.byref(ln)) == 0 and ln.value == L
    assert np.array_equal(ids, dcp.random_seq(seed, 0, L, probs))
    for q in (1, n - 1):
        assert np.array_equal(a.fetch_seq(q), dcp.random_seq(seed, q, L, probs))
    assert same_matrices(a.forward_scores(), b.forward_scores())
    for x, y in zip(a.fit_exp_tail(k), got):
        assert same_bits(x, y)
    assert a.forward_dense_kernel_ms() > 0 and a.exp_tail_kernel_ms(0) > 0 and a.exp_tail_kernel_ms(1) > 0
    assert a.calib_tail_kernel_ms(0) < 0 and a.calib_tail_kernel_ms(1) < 0  # the Gumbel tail fit's clock gains nothing
    # a bad argument is refused before anything happens: the batch and the matrices stay
    kept = a.forward_scores()
    for bad_n, bad_k in ((0, 2), (n, 1), (n, n + 1), (50, 51)):
        with pytest.raises(dcp.DcpError) as e:
            a.calibrate_forward(bad_n, L, seed, bad_k)
        assert e.value.rc == dcp.RC_EINVAL and a.nseqs == n
    out5 = [np.zeros(65), np.zeros(65), np.zeros(65, np.uint8), np.zeros(65), np.zeros(65, np.uint32)]
    for i in range(5):
        args = [x.ctypes.data for x in out5]
        args[i] = None
        assert a._lib.dcp_gpu_db_calibrate_forward(a._c, 10, L, seed, None, 1, 0, 2, *args) == dcp.RC_EINVAL
        assert "null output" in a._lib.dcp_gpu_last_error(a._c).decode() and a.nseqs == n
    assert same_matrices(a.forward_scores(), kept)
    a.close()
    b.close()


# ---- E-values end to end -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_evalues_of_the_planted_genes(dcp, oracle32, oracle64, precision):
    """The planted world: one 6 000-nt sequence with a copy of profiles 0 and 1 on the plus strand and of profile 2 on the
    minus strand.  Calibrated at 6 000 nt, every planted (strand, profile) has a Forward E-value below every other pair's,
    and below 1.  No magnitude is asserted."""
    profs, _, seq, _ = planted_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    mu, lam, st, tau, k_eff = sc.calibrate_forward(256, PLANT_L, 2027, 64)
    assert (st == dcp.FIT_OK).all() and (lam > 0).all()
    sc.upload_seqs([seq])
    sc.add_reverse_strand()
    sq, pr_ = full_list(sc)
    null, alt = sc.forward_pairs(sq, pr_)
    e = dcp.score_evalues(pr_, null, alt, mu, lam, st, sc.nseqs, dcp.LAW_EXP)
    planted = np.array([(q, p) in ((0, 0), (0, 1), (1, 2)) for q, p in zip(sq, pr_)])
    fin = np.isfinite(alt) & np.isfinite(null)
    assert fin[planted].all() and (fin & ~planted).sum() >= 1 and not np.isnan(e[fin]).any()
    print("f%d: planted E-values %s, the others %s; score - tau: planted %s, others %s" % (
        precision, e[planted], e[fin & ~planted], (alt - null - tau[pr_])[planted], (alt - null - tau[pr_])[fin & ~planted]))
    assert e[planted].max() < e[fin & ~planted].min() and e[planted].max() < 1.0
    sc.close()
