"""The censored (tail) Gumbel fit: dcp_gumbel_fit_tail on the host (csrc/dcp_model.cpp) and tail_select_kernel /
gumbel_fit_tail_kernel (csrc/dcp_calib.hip) behind dcp_gpu_fit_gumbel_tail / dcp_gpu_db_calibrate_tail on the device.
The rule is csrc/dcp_calib.h: tau = the k-th largest score by value, the k_eff scores >= tau enter with their values
and the other n - k_eff only as "below tau"; double arithmetic, every sum in index order, exactly 12 Newton steps.

The bound is test_gumbel_fit.py's, whose derivation carries over: the sums' terms are non-negative and in the same
order on both sides (the censored scores add the exact integer z = n - k_eff to s0), and |df| >= 1 / lambda^2 still holds
because s2 / s0 - r^2 is a weighted variance.  |d lambda| <= 2^-32 lambda, |d mu| <= 2^-32 (|mu| + 1 / lambda); tau, k_eff and
the status are compared exactly -- the selection only compares.

CPU: the host twin against a numpy restatement on the oracle's scores; k = n against dcp_gumbel_fit in bits; ties;
     permutations; statuses, strides, refusals; the likelihood equation's residual on Gumbel samples; a glued sample;
     tests/c/asan_calib_tail.c under ASan + UBSan as a program of its own.
GPU: the device against the host twin on scores() of the same scan at the lane edges; k = N against fit_gumbel() in
     bits; tied rows; a NONFINITE lane among others; calibrate_tail() against its three steps; the refusals."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, hit_fields
from test_c_host import ROOT
from test_gumbel_fit import (FIT_M, FIT_SEEDS, FIT_SHAPES, LANE_N, LANE_NPROF, PRECISIONS, REL, lane_profiles, oracle_scores,
                             seqsum, within_bound)


def tail_counts(n):
    """k = 2, 3, n / 4, n - 1, n where valid, each once"""
    return sorted({k for k in (2, 3, n // 4, n - 1, n) if 2 <= k <= n})


def np_fit_tail(x, k, trace=None):
    """the rule as stated: (mu, lambda, status, tau, k_eff)"""
    x = np.asarray(x, np.float64)
    n = len(x)
    assert 2 <= k <= n
    if not np.isfinite(x).all():
        return np.nan, np.nan, 17, np.nan, 0
    with np.errstate(all="ignore"):
        tau = np.sort(x)[n - k]
        obs = x >= tau
        k_eff = int(obs.sum())
        z = float(n - k_eff)
        mean = seqsum(x) / n
        var = seqsum((x - mean) * (x - mean)) / (n - 1)
        if var == 0:
            return np.nan, np.nan, 16, tau, k_eff
        lam = np.pi / np.sqrt(6.0 * var)
        xo = x[obs]  # index order
        gap = seqsum(xo) / k_eff - tau
        if gap == 0:
            return np.nan, np.nan, 16, tau, k_eff
        y = xo - tau
        diverged, settled = False, False
        for _ in range(12):
            w = np.exp(-(lam * y))
            s0, s1, s2 = seqsum(w) + z, seqsum(y * w), seqsum((y * y) * w)
            r = s1 / s0
            f = 1.0 / lam - gap + r
            df = -1.0 / (lam * lam) - s2 / s0 + r * r
            nxt = lam - f / df
            if not np.isfinite(nxt) or not nxt > 0:
                diverged, nxt = True, lam
            settled = abs(nxt - lam) <= 2.0 ** -40 * nxt
            if trace is not None:
                trace.append(abs(nxt - lam) / nxt)
            lam = nxt
        if diverged or not settled:
            return np.nan, np.nan, 18, tau, k_eff
        return tau - np.log((seqsum(np.exp(-(lam * y))) + z) / k_eff) / lam, lam, 0, tau, k_eff


def residual(x, lam, tau):
    """f(lambda) of the likelihood equation, recomputed from the sample"""
    y = x[x >= tau] - tau
    w = np.exp(-lam * y)
    return 1.0 / lam - y.mean() + (y * w).sum() / (w.sum() + (len(x) - len(y)))


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


# ---- CPU: the twin against the restatement -----------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_tail_twin_equals_the_restatement_on_oracle_scores(dcp, oracle32, oracle64, precision):
    """The profiles, shapes and seeds of test_twin_equals_the_restatement_on_oracle_scores, k = 2, 3, n / 4, n - 1, n.
    Not every one of these fits is DCP_FIT_OK: from the whole sample's moment estimate, Newton on a tail of two or three
    scores (and now and then of n / 4) overshoots to a lambda <= 0 or has not settled after 12 steps -- DIVERGED, on both
    sides alike (about one fit in eleven here; a few tails of two tie and are FLAT).  Every case is run: tau, k_eff and the status must agree exactly on all
    of them, and mu and lambda within the bound wherever the restatement is OK, which every k = n fit must be."""
    oracle = oracle64 if precision == 64 else oracle32
    worst_l = worst_m = 0.0
    slowest = fits = 0
    diverged = collections.Counter()
    for seed in FIT_SEEDS:
        for shape in FIT_SHAPES:
            x = oracle_scores(dcp, oracle, precision, seed, shape)
            n = shape[0]
            for p in range(len(FIT_M)):
                col = x[:, p]
                for k in tail_counts(n):
                    where = (precision, seed, shape, FIT_M[p], k)
                    steps = []
                    wm, wl, ws, wt, wk = np_fit_tail(col, k, steps)
                    gm, gl, gs, gt, gk = dcp.gumbel_fit_tail(col, k)  # a column: stride len(FIT_M)
                    assert (gs, gk) == (ws, wk) and bits(np.float64(gt)) == bits(np.float64(wt)), where
                    assert wk >= k and (col >= wt).sum() == wk and (col > wt).sum() < k, where
                    assert same_bits(dcp.gumbel_fit_tail(np.ascontiguousarray(col), k), (gm, gl, gs, gt, gk)), where
                    fits += 1
                    if k == n:  # the whole-sample fit: test_gumbel_fit.py's premise, every one converges
                        assert ws == dcp.FIT_OK, where
                    if ws != dcp.FIT_OK:
                        assert np.isnan(gm) and np.isnan(gl), where
                        if ws == dcp.FIT_FLAT:  # the tail's scores tie
                            assert (col[col >= wt] == wt).all() and wk < n, where
                        else:
                            assert ws == dcp.FIT_DIVERGED, where
                        diverged[k if k <= 3 else "n/4" if k == n // 4 else "n-1"] += 1
                        continue
                    slowest = max(slowest, 1 + next(i for i, d in enumerate(steps) if d < 1e-14))
                    ok, dl, dm = within_bound((gm, gl), (wm, wl))
                    assert wl > 0 and ok, (where, dl, dm)
                    worst_l, worst_m = max(worst_l, dl), max(worst_m, dm)
    print("precision %d: %d tail fits, twin vs restatement, max |d lambda| / lambda = %.3g, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % (precision, fits, worst_l, worst_m))
    print("precision %d: DIVERGED or FLAT on both sides, by k: %s; the slowest OK fit took %d of the 12 steps to a relative step "
          "below 1e-14" % (precision, dict(diverged), slowest))
    assert sum(diverged.values()) < fits // 2  # most fits are OK: the bound was looked at


def test_k_equals_n_is_the_whole_sample_fit(dcp):
    rng = np.random.default_rng(29)
    samples = [rng.gumbel(-3.0, 2.5, n) for n in (2, 3, 5, 64, 200, 1000)]
    samples += [rng.normal(0.0, 4.0, 77), np.array([0.0, 1e200, 3e200]), np.full(8, 3.75), np.array([1.0, np.inf, 2.0]),
                np.array([-0.0, 0.0, 1.5, 0.25]), np.array([0.0, -0.0, 1.5, 0.25]), rng.gumbel(0.0, 1.0, 50).round(1)]
    seen = set()
    for x in samples:
        n = len(x)
        mu, lam, st = dcp.gumbel_fit(x)
        tm, tl, ts, tau, k_eff = dcp.gumbel_fit_tail(x, n)
        seen.add(st)
        assert ts == st and same_bits([tm, tl], [mu, lam]), x
        if st == dcp.FIT_NONFINITE:
            assert np.isnan(tau) and k_eff == 0
        else:
            assert tau == x.min() and k_eff == n
    assert seen == {dcp.FIT_OK, dcp.FIT_FLAT, dcp.FIT_NONFINITE, dcp.FIT_DIVERGED}
    # strided too
    mat = rng.gumbel(0.0, 1.0, (50, 7))
    for p in range(7):
        assert dcp.gumbel_fit_tail(mat[:, p], 50)[:3] == dcp.gumbel_fit(mat[:, p])


def test_ties_widen_the_tail(dcp):
    rng = np.random.default_rng(31)
    x = rng.gumbel(2.0, 1.5, 120)
    order = np.argsort(x)[::-1]
    # the values at ranks 10 .. 14 (from the top, 1-based) all become the value at rank 10
    x[order[10:14]] = x[order[9]]
    t = x[order[9]]
    for k in (10, 11, 12, 13, 14):
        mu, lam, st, tau, k_eff = dcp.gumbel_fit_tail(x, k)
        assert (st, tau, k_eff) == (dcp.FIT_OK, t, 14), k
        assert same_bits([mu, lam], dcp.gumbel_fit_tail(x, 14)[:2])
        assert np_fit_tail(x, k)[2:] == (st, tau, k_eff)
        assert within_bound((mu, lam), np_fit_tail(x, k)[:2])[0]
    assert dcp.gumbel_fit_tail(x, 9)[3:] == (x[order[8]], 9)
    assert dcp.gumbel_fit_tail(x, 15)[3:] == (x[order[14]], 15)
    # zeros of either sign are one value
    z = np.array([3.0, -0.0, 0.0, -1.0, 0.0, -2.5, 7.0, -0.0])
    for k, (tau, k_eff) in {2: (3.0, 2), 3: (0.0, 6), 6: (0.0, 6), 7: (-1.0, 7), 8: (-2.5, 8)}.items():
        got = dcp.gumbel_fit_tail(z, k)
        assert got[3] == tau and got[4] == k_eff, (k, got)


def test_a_permutation_keeps_tau_and_k_eff(dcp):
    rng = np.random.default_rng(37)
    x = rng.gumbel(-5.0, 0.8, 200).round(1)  # rounded: ties throughout
    assert len(np.unique(x)) < 100
    for k in (2, 3, 50, 100, 199, 200):
        base = dcp.gumbel_fit_tail(x, k)
        assert base[2] == dcp.FIT_OK and base[3:] == np_fit_tail(x, k)[3:]
        for _ in range(5):
            y = rng.permutation(x)
            got = dcp.gumbel_fit_tail(y, k)
            assert got[2] == dcp.FIT_OK and got[3:] == base[3:], k
            assert within_bound(got[:2], base[:2])[0]  # the sums' order moved: the last bits may
        assert dcp.gumbel_fit_tail(x[::-1], k)[3:] == base[3:]


def test_tail_statuses_strides_and_refusals(dcp):
    rng = np.random.default_rng(41)
    x = rng.gumbel(-3.0, 2.5, 400)
    mu, lam, st, tau, k_eff = dcp.gumbel_fit_tail(x, 100)
    assert st == dcp.FIT_OK and k_eff == 100 and tau == np.sort(x)[300] and abs(lam - 0.4) < 0.1 and abs(mu + 3.0) < 1.0
    assert within_bound((mu, lam), np_fit_tail(x, 100)[:2])[0]
    # every observed value equal to tau, k < n: FLAT, with tau and k_eff
    for flat, k, k_eff in ((np.array([1.0, 3.75, 2.0, 3.75, 0.5]), 2, 2), (np.array([-7.25, -9.0, -7.25, -7.25, -7.25, -8.0]), 3, 4),
                           (np.array([0.5, 0.5, 0.25]), 2, 2)):
        got = dcp.gumbel_fit_tail(flat, k)
        assert got[2] == dcp.FIT_FLAT == np_fit_tail(flat, k)[2] and np.isnan(got[0]) and np.isnan(got[1]), flat
        assert got[3] == flat.max() and got[4] == k_eff
    # no variance at all
    for flat in (np.zeros(5), np.full(8, 3.75)):
        for k in (2, len(flat)):
            got = dcp.gumbel_fit_tail(flat, k)
            assert got[2] == dcp.FIT_FLAT and np.isnan(got[0]) and np.isnan(got[1]) and got[3:] == (flat[0], len(flat))
    # one non-finite value, anywhere
    for bad in (-np.inf, np.inf, np.nan):
        for at in (0, 200, 399):
            y = x.copy()
            y[at] = bad
            for k in (2, 100, 400):
                mu, lam, st, tau, k_eff = dcp.gumbel_fit_tail(y, k)
                assert st == dcp.FIT_NONFINITE == np_fit_tail(y, k)[2] and k_eff == 0, (bad, at, k)
                assert np.isnan(mu) and np.isnan(lam) and np.isnan(tau)
    # a variance that overflows: lambda starts at 0 and no step leaves it finite and positive
    for wild in (np.array([0.0, 1e200, 3e200]), np.array([-1e308, 1e308, 0.0])):
        for k in (2, 3):
            mu, lam, st, tau, k_eff = dcp.gumbel_fit_tail(wild, k)
            assert st == dcp.FIT_DIVERGED == np_fit_tail(wild, k)[2] and np.isnan(mu) and np.isnan(lam)
            assert (tau, k_eff) == (np.sort(wild)[3 - k], k)
    # strides: every third value, and a column of a matrix
    assert dcp.gumbel_fit_tail(x[::3], 30) == dcp.gumbel_fit_tail(x[::3].copy(), 30)
    mat = rng.gumbel(0.0, 1.0, (50, 7))
    for p in range(7):
        assert dcp.gumbel_fit_tail(mat[:, p], 12) == dcp.gumbel_fit_tail(mat[:, p].copy(), 12)
    # the refusals: nothing written
    for k in (0, 1, 401):
        with pytest.raises(dcp.DcpError) as e:
            dcp.gumbel_fit_tail(x, k)
        assert e.value.rc == dcp.RC_EINVAL
    for n in (0, 1):
        with pytest.raises(dcp.DcpError):
            dcp.gumbel_fit_tail(x[:n], 2)
    out = [C.c_double(5.0), C.c_double(6.0), C.c_double(7.0), C.c_uint(8)]
    refs = [C.byref(o) for o in out]
    fn = dcp.lib.dcp_gumbel_fit_tail
    for n, stride, k in ((10, 1, 0), (10, 1, 1), (10, 1, 11), (1, 1, 2), (0, 1, 2), (10, 0, 5)):
        assert fn(x.ctypes.data, n, stride, k, *refs) == dcp.RC_EINVAL
    assert fn(None, 10, 1, 5, *refs) == dcp.RC_EINVAL
    for i in range(4):
        args = list(refs)
        args[i] = None
        assert fn(x.ctypes.data, 10, 1, 5, *args) == dcp.RC_EINVAL
    assert [o.value for o in out] == [5.0, 6.0, 7.0, 8]
    assert fn(x.ctypes.data, 10, 1, 5, *refs) == dcp.FIT_OK and out[3].value == 5


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_the_fit_solves_the_likelihood_equation(dcp, seed):
    """n = 1 000 Gumbel scores, k = 100: a step settled to 2^-40 leaves |f| ~ |df| |d lambda|, a few 2^-40 / lambda."""
    rng = np.random.default_rng(seed)
    lam0, mu0 = (0.3, 0.7, 1.3, 2.0)[seed - 1], (-7.0, 0.0, 4.0, 30.0)[seed - 1]
    x = rng.gumbel(mu0, 1.0 / lam0, 1000)
    mu, lam, st, tau, k_eff = dcp.gumbel_fit_tail(x, 100)
    assert st == dcp.FIT_OK and k_eff == 100 and tau == np.sort(x)[900]
    f = residual(x, lam, tau)
    print("seed %d: lambda %.4f (drawn with %.1f), mu %.3f (%.1f), |f| lambda = %.3g" % (seed, lam, lam0, mu, mu0, abs(f) * lam))
    assert abs(f) <= 2.0 ** -30 / lam
    # mu solves its equation too: sum over the tail of exp(-lambda (x - mu)) + z exp(-lambda (tau - mu)) = k_eff
    tail = x[x >= tau]
    g = np.exp(-lam * (tail - mu)).sum() + (len(x) - k_eff) * np.exp(-lam * (tau - mu))
    assert abs(g / k_eff - 1.0) < 1e-12
    assert abs(lam - lam0) < 0.35 * lam0  # a hundred points: the law is recovered roughly


def test_a_glued_sample_has_a_steeper_tail(dcp):
    """800 normal scores with 200 Gumbel(-7, lambda = 1.3) scores glued on: the whole-sample fit spends its likelihood on
    the bulk, the tail fit reads the tail."""
    rng = np.random.default_rng(2026)
    x = np.concatenate([rng.normal(-12.0, 2.0, 800), rng.gumbel(-7.0, 1.0 / 1.3, 200)])
    x = rng.permutation(x)
    whole = dcp.gumbel_fit_tail(x, 1000)
    tail = dcp.gumbel_fit_tail(x, 50)
    print("glued sample: lambda %.3f with k = n, %.3f with k = 100, %.3f with k = 50"
          % (whole[1], dcp.gumbel_fit_tail(x, 100)[1], tail[1]))
    assert whole[2] == tail[2] == dcp.FIT_OK and tail[4] == 50
    assert same_bits(whole[:2], dcp.gumbel_fit(x)[:2])
    assert tail[1] > whole[1]


def test_calib_tail_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_calib_tail.c with the host model alone (no device code) under ASan + UBSan, as a program of its
    own."""
    obj, exe = str(tmp_path / "asan_calib_tail.o"), str(tmp_path / "asan_calib_tail")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_calib_tail.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_calib_tail ok" in r.stdout


# ---- GPU: the device against the host twin -----------------------------------------------------------------------

def host_tail_fits(dcp, sc, k):
    """the host twin on scores() of the scan that is resident: (mu, lam, status, tau, k_eff) arrays"""
    null, alt = sc.scores()
    with np.errstate(invalid="ignore"):  # -inf - -inf of an epsilon = 0 lane
        x = alt.astype(np.float64) - null.astype(np.float64)
    fits = [dcp.gumbel_fit_tail(x[:, p], k) for p in range(x.shape[1])]
    return (np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[2] for f in fits], np.uint8),
            np.array([f[3] for f in fits]), np.array([f[4] for f in fits], np.uint32))


def compare_tail_fits(got, want, where):
    """tau, k_eff and statuses equal, NaN where not OK, lambda and mu within the bound: the two maxima"""
    (gm, gl, gs, gt, gk), (wm, wl, ws, wt, wk) = got, want
    assert gs.dtype == np.uint8 and np.array_equal(gs, ws), (where, gs, ws)
    assert gk.dtype == np.uint32 and np.array_equal(gk, wk), (where, gk, wk)
    assert same_bits(gt, wt), (where, gt, wt)
    ok = ws == 0
    assert np.isnan(gm[~ok]).all() and np.isnan(gl[~ok]).all(), where
    if not ok.any():
        return 0.0, 0.0
    dl = np.abs(gl[ok] - wl[ok]) / wl[ok]
    dm = np.abs(gm[ok] - wm[ok]) / (np.abs(wm[ok]) + 1.0 / wl[ok])
    assert (gl[ok] > 0).all() and dl.max() <= REL and dm.max() <= REL, (where, dl.max(), dm.max())
    return float(dl.max()), float(dm.max())


@pytest.mark.gpu
@pytest.mark.parametrize("nprof", LANE_NPROF)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_tail_fit_equals_the_host_twin(dcp, precision, nprof):
    sc = dcp.Scanner(0)
    sc.upload_db(lane_profiles(dcp, precision, nprof))
    worst = (0.0, 0.0)
    for n in LANE_N:
        sc.random_seqs(n, 100, 40 + n)
        sc.scan(True, False, 10.0)
        whole = sc.fit_gumbel()
        for k in tail_counts(n):
            got = sc.fit_gumbel_tail(k)
            want = host_tail_fits(dcp, sc, k)
            assert (got[4] >= k).all() and (got[4] <= n).all()
            worst = tuple(max(a, b) for a, b in zip(worst, compare_tail_fits(got, want, (precision, nprof, n, k))))
            if k == n:  # the whole-sample fit of the same scan, in bits
                assert np.array_equal(got[2], whole[2]) and same_bits(got[0], whole[0]) and same_bits(got[1], whole[1])
                assert (got[4] == n).all()
        for x, y in zip(sc.fit_gumbel(), whole):  # the scan's results stay valid
            assert same_bits(x, y)
    print("precision %d, %d profiles: device vs host twin, max |d lambda| / lambda = %.3g, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % ((precision, nprof) + worst))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tied_rows_on_the_device(dcp, precision):
    """Repeated sequences: whole rows of scores are equal.  Four and two copies sum and divide exactly, so a tail that
    is one value has gap == 0."""
    profs = lane_profiles(dcp, precision, 70)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    a, b, c = (dcp.random_seq(11, q, 100) for q in range(3))
    # four copies of a, four of b, interleaved
    sc.upload_seqs([a, b, a, b, b, a, b, a])
    sc.scan(True, False, 10.0)
    null, alt = sc.scores()
    x = alt.astype(np.float64) - null.astype(np.float64)
    assert np.array_equal(x[0], x[2]) and np.array_equal(x[1], x[4]) and (x[0] != x[1]).sum() >= 60
    for k in (2, 3, 4):
        mu, lam, st, tau, k_eff = sc.fit_gumbel_tail(k)
        assert np.array_equal(k_eff, np.where(x[0] != x[1], 4, 8))  # (a profile that scores a and b alike: all eight)
        assert np.array_equal(tau, x.max(axis=0)) and (st == dcp.FIT_FLAT).all()
        assert np.isnan(mu).all() and np.isnan(lam).all()
        compare_tail_fits((mu, lam, st, tau, k_eff), host_tail_fits(dcp, sc, k), (precision, k))
    for k in (5, 8):
        got = sc.fit_gumbel_tail(k)
        assert (got[4] == 8).all() and np.array_equal(got[3], x.min(axis=0))
        compare_tail_fits(got, host_tail_fits(dcp, sc, k), (precision, k))
    # a: 4, b: 2, c: 2, and six sequences of their own
    sc.upload_seqs([a, c, b, a] + [dcp.random_seq(12, q, 100) for q in range(6)] + [a, b, c, a])
    sc.scan(True, False, 10.0)
    null, alt = sc.scores()
    x = alt.astype(np.float64) - null.astype(np.float64)
    n = len(x)
    flat = 0
    for k in range(2, n + 1):
        got = sc.fit_gumbel_tail(k)
        tau = np.sort(x, axis=0)[n - k]
        assert np.array_equal(got[3], tau) and np.array_equal(got[4], (x >= tau).sum(axis=0))
        all_tied = (np.where(x >= tau, x, tau) == tau).all(axis=0) & (got[4] < n)
        assert (got[2][all_tied] == dcp.FIT_FLAT).all()
        flat += int(all_tied.sum())
        compare_tail_fits(got, host_tail_fits(dcp, sc, k), (precision, k))
    assert flat > 0
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_nonfinite_lane_leaves_its_neighbours_alone(dcp, precision):
    profs = lane_profiles(dcp, precision, 70)
    at, n, k = 37, 64, 16
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.random_seqs(n, 100, 5)
    sc.scan(True, False, 10.0)
    base = sc.fit_gumbel_tail(k)
    assert (base[2] == dcp.FIT_OK).sum() >= 60 and (base[4] >= k).all()
    zero = dcp.ProteinProfile.sample(999, 40, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    sc.upload_db(profs[:at] + [zero] + profs[at:])
    sc.random_seqs(n, 100, 5)
    sc.scan(True, False, 10.0)
    null, alt = sc.scores()
    assert not (np.isfinite(alt[:, at]) & np.isfinite(null[:, at])).all()
    mu, lam, st, tau, k_eff = sc.fit_gumbel_tail(k)
    assert st[at] == dcp.FIT_NONFINITE and np.isnan(mu[at]) and np.isnan(lam[at]) and np.isnan(tau[at]) and k_eff[at] == 0
    rest = np.arange(len(profs) + 1) != at
    assert np.array_equal(st[rest], base[2]) and np.array_equal(k_eff[rest], base[4])
    assert same_bits(mu[rest], base[0]) and same_bits(lam[rest], base[1]) and same_bits(tau[rest], base[3])
    compare_tail_fits((mu, lam, st, tau, k_eff), host_tail_fits(dcp, sc, k), precision)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,kernel", [(32, 1), (32, 2), (32, 3), (64, 1), (64, 4)])
def test_calibrate_tail_is_its_three_steps(dcp, precision, kernel):
    profs = lane_profiles(dcp, precision, 65)
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    n, L, seed, k, probs = 80, 90, 77, 20, (0.3, 0.2, 0.2, 0.3)
    a._check(a._lib.dcp_gpu_set_lrt_threshold64(a._c, -1e300))  # a double DB's own threshold: restored behind the scan
    got = a.calibrate_tail(n, L, seed, k, probs, multi_hits=True, hmmer3_compat=False, kernel=kernel)
    b.random_seqs(n, L, seed, probs)
    b.scan(True, False, float("inf"), keep_scores=True, kernel=kernel)
    want = b.fit_gumbel_tail(k)
    assert len(got) == 5 and got[4].dtype == np.uint32
    for x, y in zip(got, want):
        assert same_bits(x, y), (precision, kernel)
    assert (got[2] == dcp.FIT_OK).sum() >= 0.9 * len(profs), got[2]
    assert (got[4] >= k).all()
    # what it leaves: the random batch and that scan
    assert (a.nseqs, a.strands, a.windows) == (n, 1, None) and a.last_scan_kernel == b.last_scan_kernel
    for q in (0, 1, n - 1):
        assert np.array_equal(a.fetch_seq(q), dcp.random_seq(seed, q, L, probs))
    for x, y in zip(a.scores(), b.scores()):
        assert np.array_equal(bits(x), bits(y))
    assert len(a.hits()) == 0 and len(b.hits()) == 0
    for x, y in zip(a.fit_gumbel_tail(k), got):
        assert same_bits(x, y)
    assert a.calib_tail_kernel_ms(0) > 0 and a.calib_tail_kernel_ms(1) > 0 and a.calib_tail_kernel_ms(2) < 0
    if precision == 64:  # the caller's threshold is in force again: a raw scan reports every finite pair
        prm = dcp.ScanParams(1, 0, float("inf"), 1, 1)
        a._check(a._lib.dcp_gpu_scan(a._c, C.byref(prm)))
        a.sync()
        assert len(a.hits()) == n * len(profs)
    # a bad argument is refused before anything happens, and the batch stays
    for bad_n, bad_k in ((0, 2), (n, 1), (n, n + 1), (50, 51)):
        with pytest.raises(dcp.DcpError) as e:
            a.calibrate_tail(bad_n, L, seed, bad_k)
        assert e.value.rc == dcp.RC_EINVAL and a.nseqs == n
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_of_the_tail_fit(dcp, precision):
    profs = lane_profiles(dcp, precision, 10)
    rng = np.random.default_rng(precision)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(40, 200, 12)]
    sc = dcp.Scanner(0)
    assert sc.calib_tail_kernel_ms(0) < 0 and sc.calib_tail_kernel_ms(1) < 0
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    mu, lam, st = np.full(10, 9.0), np.full(10, 9.0), np.full(10, 9, np.uint8)
    tau, k_eff = np.full(10, 9.0), np.full(10, 9, np.uint32)
    ptr = lambda a: a.ctypes.data

    def refused(k, *words):
        assert sc._lib.dcp_gpu_fit_gumbel_tail(sc._c, k, ptr(mu), ptr(lam), ptr(st), ptr(tau), ptr(k_eff)) == dcp.RC_EINVAL
        msg = sc._lib.dcp_gpu_last_error(sc._c).decode()
        assert all(w in msg for w in words), msg
        assert (mu == 9.0).all() and (lam == 9.0).all() and (st == 9).all() and (tau == 9.0).all() and (k_eff == 9).all()

    refused(4, "no scan")
    sc.scan(True, False, 10.0, keep_scores=True)
    want = [bits(x).copy() for x in sc.scores()]
    want_hits = hit_fields(sc.hits())
    ok = sc.fit_gumbel_tail(4)
    assert (ok[2] == dcp.FIT_OK).any()
    for k in (0, 1, 13, 2 ** 32 - 1):
        refused(k, "tail count", "12")
    for i in range(5):
        args = [ptr(mu), ptr(lam), ptr(st), ptr(tau), ptr(k_eff)]
        args[i] = None
        assert sc._lib.dcp_gpu_fit_gumbel_tail(sc._c, 4, *args) == dcp.RC_EINVAL
        assert "null output" in sc._lib.dcp_gpu_last_error(sc._c).decode()
    sc.scan(True, False, 10.0, keep_scores=False)
    refused(4, "dense scores")
    sc.scan_pairs([0, 1], [1, 2])
    refused(4, "dense scores")
    sc.scan(True, False, 10.0, q_range=(0, 11))
    refused(4, "whole batch")
    sc.scan(True, False, 10.0, q_range=(1, 12))
    refused(4, "whole batch")
    sc.upload_seqs(seqs[:1])
    refused(2, "no scan")
    sc.scan(True, False, 10.0)
    refused(2, "2 sequences")
    with pytest.raises(dcp.DcpError) as e:
        sc.fit_gumbel_tail(2)
    assert e.value.rc == dcp.RC_EINVAL
    # a normal scan behind a tail calibration is what it was
    sc.calibrate_tail(50, 60, 1, 10)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0, keep_scores=True)
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    assert hit_fields(sc.hits()) == want_hits
    for x, y in zip(sc.fit_gumbel_tail(4), ok):
        assert same_bits(x, y)
    sc.close()
