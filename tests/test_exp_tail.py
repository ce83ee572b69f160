"""The exponential tail fit on the host: dcp_exp_tail_fit, dcp_exp_sf and dcp_scores_evalues (csrc/dcp_model.cpp; the
rule is csrc/dcp_calib.h: tau = the k-th largest score by value, lambda = k_eff / sum over the k_eff scores >= tau of
(x - tau) in index order, mu = tau + log(k_eff / n) / lambda).

tau, k_eff, the status and lambda are compared in bits with a numpy restatement: comparisons, one ordered sum, one
division.  mu lies behind one log and one division more: |d mu| <= 2^-32 (|mu| + 1 / lambda), test_gumbel_fit.py's bound.

The twin against the restatement on the oracle's scores; k = n; strides; permutations; statuses; refusals; exponential
samples against five standard errors of the estimator; the survival function; score_evalues against hit_evalues;
tests/c/asan_exp_tail.c under ASan + UBSan as a program of its own.  (The device: test_forward_dense.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_c_host import ROOT
from test_gumbel_fit import FIT_M, FIT_SEEDS, FIT_SHAPES, PRECISIONS, REL, oracle_scores, seqsum
from test_gumbel_tail import same_bits, tail_counts


def np_exp_tail(x, k):
    """the rule as stated: (mu, lambda, status, tau, k_eff)"""
    x = np.asarray(x, np.float64)
    n = len(x)
    assert 2 <= k <= n
    if not np.isfinite(x).all():
        return np.nan, np.nan, 17, np.nan, 0
    tau = np.sort(x)[n - k]
    obs = x >= tau
    k_eff = int(obs.sum())
    so = seqsum(x[obs] - tau)  # index order
    if so == 0:
        return np.nan, np.nan, 16, tau, k_eff
    lam = k_eff / so
    return tau + np.log(k_eff / n) / lam, lam, 0, tau, k_eff


def mu_within_bound(got, want, lam):
    d = abs(got - want) / (abs(want) + 1.0 / lam)
    return d <= REL, d


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exp_twin_equals_the_restatement_on_oracle_scores(dcp, oracle32, oracle64, precision):
    """The profiles, shapes and seeds of test_gumbel_fit.py, k = 2, 3, n / 4, n - 1, n.  The premise first, read off the
    columns themselves: every column is finite, and a fit is OK unless the column's k largest scores are one value.  They
    are not all untied -- the oracle scores some generator sequences alike, and in 3 of the 1008 cases (two float, one
    double, all k = 2) the two best scores of a column tie: the whole observed set sits at tau, FLAT on both sides.  Every
    case is run; no other status occurs."""
    oracle = oracle64 if precision == 64 else oracle32
    worst = 0.0
    fits = flat = 0
    for seed in FIT_SEEDS:
        for shape in FIT_SHAPES:
            x = oracle_scores(dcp, oracle, precision, seed, shape)
            n = shape[0]
            for p in range(len(FIT_M)):
                col = x[:, p]
                assert np.isfinite(col).all(), (precision, seed, shape, FIT_M[p])
                for k in tail_counts(n):
                    where = (precision, seed, shape, FIT_M[p], k)
                    top = np.sort(col)[n - k:]
                    premise = dcp.FIT_FLAT if top[0] == top[-1] else dcp.FIT_OK
                    wm, wl, ws, wt, wk = np_exp_tail(col, k)
                    assert ws == premise and wk >= k and (col >= wt).sum() == wk and (col > wt).sum() < k, where
                    gm, gl, gs, gt, gk = dcp.exp_tail_fit(col, k)  # a column: stride len(FIT_M)
                    assert (gs, gk) == (ws, wk) and same_bits(gt, wt) and same_bits(gl, wl), where
                    assert same_bits(dcp.exp_tail_fit(np.ascontiguousarray(col), k), (gm, gl, gs, gt, gk)), where
                    assert dcp.gumbel_fit_tail(col, k)[3:] == (gt, gk), where  # the selection is the Gumbel tail fit's
                    fits += 1
                    if ws == dcp.FIT_FLAT:
                        assert np.isnan(gm) and np.isnan(gl) and k == 2, where
                        flat += 1
                        continue
                    ok, d = mu_within_bound(gm, wm, wl)
                    assert gl > 0 and ok, (where, d)
                    worst = max(worst, d)
    print("precision %d: %d fits (%d FLAT: the two best scores tie), twin vs restatement: tau, k_eff, status, lambda in bits; "
          "max |d mu| / (|mu| + 1 / lambda) = %.3g" % (precision, fits, flat, worst))
    assert flat <= 2  # the premise as counted above


def test_k_equals_n_puts_mu_at_the_minimum(dcp):
    rng = np.random.default_rng(29)
    for x in [rng.exponential(2.0, n) - 3.0 for n in (2, 3, 5, 64, 200, 1000)] + [rng.normal(0.0, 4.0, 77),
                                                                               np.array([-0.0, 0.0, 1.5, 0.25])]:
        mu, lam, st, tau, k_eff = dcp.exp_tail_fit(x, len(x))
        assert st == dcp.FIT_OK and k_eff == len(x) and tau == x.min()
        assert same_bits(mu, tau + 0.0) and lam > 0  # log(n / n) = 0: mu is tau itself
        assert same_bits(lam, len(x) / seqsum(x - tau))


def test_strides_and_permutations(dcp):
    rng = np.random.default_rng(37)
    x = rng.exponential(0.8, 400) - 5.0
    assert same_bits(dcp.exp_tail_fit(x[::3], 30), dcp.exp_tail_fit(x[::3].copy(), 30))
    mat = rng.exponential(1.0, (50, 7))
    for p in range(7):
        assert same_bits(dcp.exp_tail_fit(mat[:, p], 12), dcp.exp_tail_fit(mat[:, p].copy(), 12))
    y = x[:200].round(1)  # rounded: ties throughout
    assert len(np.unique(y)) < 100
    for k in (2, 3, 50, 100, 199, 200):
        base = dcp.exp_tail_fit(y, k)
        assert base[3:] == np_exp_tail(y, k)[3:] and base[2] == np_exp_tail(y, k)[2]
        for _ in range(5):
            got = dcp.exp_tail_fit(rng.permutation(y), k)
            assert got[2] == base[2] and got[3:] == base[3:], k
            if base[2] == dcp.FIT_OK:  # the sum's order moved: lambda's last bits may
                assert abs(got[1] - base[1]) <= REL * base[1] and mu_within_bound(got[0], base[0], base[1])[0]
        assert dcp.exp_tail_fit(y[::-1], k)[3:] == base[3:]


def test_statuses_and_refusals(dcp):
    rng = np.random.default_rng(41)
    x = rng.exponential(2.5, 400) - 3.0
    # every observed value equal to tau: FLAT, with tau and k_eff
    for flat, k, k_eff in ((np.array([1.0, 3.75, 2.0, 3.75, 0.5]), 2, 2), (np.array([-7.25, -9.0, -7.25, -7.25, -7.25, -8.0]), 3, 4),
                           (np.array([0.5, 0.5, 0.25]), 2, 2), (np.zeros(5), 2, 5), (np.full(8, 3.75), 8, 8),
                           (np.array([0.0, -0.0, -1.0]), 2, 2)):
        got = dcp.exp_tail_fit(flat, k)
        assert got[2] == dcp.FIT_FLAT == np_exp_tail(flat, k)[2] and np.isnan(got[0]) and np.isnan(got[1]), flat
        assert got[3] == flat.max() and got[4] == k_eff
    # one non-finite value, anywhere: NaN and 0
    for bad in (-np.inf, np.inf, np.nan):
        for at in (0, 200, 399):
            y = x.copy()
            y[at] = bad
            for k in (2, 100, 400):
                mu, lam, st, tau, k_eff = dcp.exp_tail_fit(y, k)
                assert st == dcp.FIT_NONFINITE == np_exp_tail(y, k)[2] and k_eff == 0, (bad, at, k)
                assert np.isnan(mu) and np.isnan(lam) and np.isnan(tau)
    # the refusals: nothing written
    for k in (0, 1, 401):
        with pytest.raises(dcp.DcpError) as e:
            dcp.exp_tail_fit(x, k)
        assert e.value.rc == dcp.RC_EINVAL
    for n in (0, 1):
        with pytest.raises(dcp.DcpError):
            dcp.exp_tail_fit(x[:n], 2)
    out = [C.c_double(5.0), C.c_double(6.0), C.c_double(7.0), C.c_uint(8)]
    refs = [C.byref(o) for o in out]
    fn = dcp.lib.dcp_exp_tail_fit
    for n, stride, k in ((10, 1, 0), (10, 1, 1), (10, 1, 11), (1, 1, 2), (0, 1, 2), (10, 0, 5)):
        assert fn(x.ctypes.data, n, stride, k, *refs) == dcp.RC_EINVAL
    assert fn(None, 10, 1, 5, *refs) == dcp.RC_EINVAL
    for i in range(4):
        args = list(refs)
        args[i] = None
        assert fn(x.ctypes.data, 10, 1, 5, *args) == dcp.RC_EINVAL
    assert [o.value for o in out] == [5.0, 6.0, 7.0, 8]
    assert fn(x.ctypes.data, 10, 1, 5, *refs) == dcp.FIT_OK and out[3].value == 5


@pytest.mark.parametrize("lam0,shift,seed", [(0.3, -7.0, 1), (0.7, 0.0, 2), (2.0, 30.0, 3)])
def test_exponential_samples_give_back_their_rate(dcp, lam0, shift, seed):
    """The excesses over tau of an exponential sample are exponential with the same rate, and lambda is k over their sum:
    its standard error is lambda / sqrt(k).  Five of them, derived, not measured."""
    n, k = 20000, 2000
    x = shift + np.random.default_rng(seed).exponential(1.0 / lam0, n)
    mu, lam, st, tau, k_eff = dcp.exp_tail_fit(x, k)
    assert st == dcp.FIT_OK and k_eff == k and tau == np.sort(x)[n - k]
    print("lambda %.4f drawn with %.1f: %.2f standard errors; mu %.3f, shift %.1f" % (lam, lam0, abs(lam - lam0) / (lam0 / np.sqrt(k)), mu, shift))
    assert abs(lam - lam0) <= 5.0 * lam0 / np.sqrt(k)
    # the law passes through the observed fraction at tau
    assert abs(dcp.exp_sf(mu, lam, tau) / (k_eff / n) - 1.0) <= 2.0 ** -40


def test_survival_function(dcp):
    for mu, lam in ((0.0, 1.0), (-12.5, 0.31), (40.0, 0.693), (3.0, 2.5)):
        for s in (mu, mu - 1e-9, mu - 10.0 / lam, -np.inf):
            assert dcp.exp_sf(mu, lam, s) == 1.0
        zs = (1e-9, 0.5, 1.0, 10.0, 40.0, 300.0, 600.0, 700.0)
        sf = [dcp.exp_sf(mu, lam, mu + z / lam) for z in zs]
        assert all(a > b > 0 for a, b in zip([1.0] + sf, sf)), sf  # strictly decreasing from 1
        # relative precision far in the tail: the argument mu + z / lam gives z back within a few ulps of |mu| lam + z
        for z, got in zip(zs, sf):
            assert abs(got - np.exp(-z)) <= (1e-12 + 4e-16 * (abs(mu) * lam + z)) * np.exp(-z), (mu, lam, z)
        assert dcp.exp_sf(mu, lam, mu + 600.0 / lam) > 1e-262
        assert dcp.exp_sf(mu, lam, np.inf) == 0.0


def test_score_evalues(dcp):
    mu, lam = np.array([1.0, 2.0, 3.0]), np.array([0.5, 0.6, 0.7])
    status = np.array([dcp.FIT_OK, dcp.FIT_NONFINITE, dcp.FIT_OK], np.uint8)
    pidx = np.array([0, 1, 2, 0], np.uint32)
    for dtype, real in ((dcp.HIT_DTYPE, np.float32), (dcp.HIT64_DTYPE, np.float64)):
        hits = np.zeros(4, dtype)
        hits["seq_idx"] = [0, 1, 2, 3]
        hits["profile_idx"] = pidx
        hits["null_loglik"] = [-100.0, -90.0, -80.0, -70.5]
        hits["alt_loglik"] = [-90.0, -85.0, -50.0, -71.0]
        null, alt = hits["null_loglik"].astype(np.float64), hits["alt_loglik"].astype(np.float64)
        # under the Gumbel law: hit_evalues' bits on the same records
        want = dcp.hit_evalues(hits, mu, lam, status, 1000.0)
        got = dcp.score_evalues(pidx, null, alt, mu, lam, status, 1000.0, dcp.LAW_GUMBEL)
        assert np.isnan(got[1]) and same_bits(got, want)
    e = dcp.score_evalues(pidx, null, alt, mu, lam, status, 1000.0, dcp.LAW_EXP)
    s = alt - null
    want = [1000.0 * dcp.exp_sf(mu[p], lam[p], v) for p, v in zip(pidx, s)]
    assert np.isnan(e[1]) and same_bits(e[[0, 2, 3]], np.array(want)[[0, 2, 3]])
    assert e[3] == 1000.0  # a score below mu: survival 1
    assert (dcp.score_evalues(pidx, null, alt, mu, lam, status, 0.0, dcp.LAW_EXP)[[0, 2, 3]] == 0).all()
    assert len(dcp.score_evalues(pidx[:0], null[:0], alt[:0], mu, lam, status, 5.0, dcp.LAW_EXP)) == 0
    assert dcp.score_evalues(pidx[:1], [0.0], [-np.inf], mu, lam, status, 7.0, dcp.LAW_EXP)[0] == 7.0  # no path at all
    for st in (dcp.FIT_FLAT, dcp.FIT_DIVERGED, dcp.FIT_NONFINITE):
        for law in (dcp.LAW_GUMBEL, dcp.LAW_EXP):
            assert np.isnan(dcp.score_evalues(pidx, null, alt, mu, lam, np.full(3, st, np.uint8), 1.0, law)).all()
    # the refusals: nothing written
    fn = dcp.lib.dcp_scores_evalues
    out = np.full(4, 9.0)
    ptr = lambda a: a.ctypes.data
    assert fn(ptr(pidx), ptr(null), ptr(alt), 4, ptr(mu), ptr(lam), ptr(status), 2, 1000.0, dcp.LAW_EXP, ptr(out)) == dcp.RC_EINVAL
    for bad in (np.nan, np.inf, -1.0):
        assert fn(ptr(pidx), ptr(null), ptr(alt), 4, ptr(mu), ptr(lam), ptr(status), 3, bad, dcp.LAW_EXP, ptr(out)) == dcp.RC_EINVAL
    for law in (-1, 2):
        assert fn(ptr(pidx), ptr(null), ptr(alt), 4, ptr(mu), ptr(lam), ptr(status), 3, 1000.0, law, ptr(out)) == dcp.RC_EINVAL
    for k in range(7):
        args = [ptr(pidx), ptr(null), ptr(alt), ptr(mu), ptr(lam), ptr(status), ptr(out)]
        args[k] = None
        assert fn(args[0], args[1], args[2], 4, args[3], args[4], args[5], 3, 1000.0, dcp.LAW_EXP, args[6]) == dcp.RC_EINVAL
    assert (out == 9.0).all()
    with pytest.raises(dcp.DcpError):
        dcp.score_evalues(pidx, null, alt, mu[:2], lam[:2], status[:2], 1000.0, dcp.LAW_EXP)
    with pytest.raises(dcp.DcpError):
        dcp.score_evalues(pidx, null, alt, mu, lam, status, -1.0, dcp.LAW_EXP)
    with pytest.raises(dcp.DcpError):
        dcp.score_evalues(pidx, null, alt, mu, lam, status, 1.0, 5)
    with pytest.raises(dcp.DcpError):
        dcp.score_evalues(pidx, null[:3], alt, mu, lam, status, 1.0, dcp.LAW_EXP)
    assert (dcp.LAW_GUMBEL, dcp.LAW_EXP, dcp.SCORES_SCAN, dcp.SCORES_FORWARD) == (0, 1, 0, 1)
    for name in ("dcp_gpu_forward_dense", "dcp_gpu_fetch_forward_scores", "dcp_gpu_forward_dense_kernel_ms", "dcp_exp_tail_fit",
                 "dcp_gpu_fit_exp_tail", "dcp_gpu_exp_tail_kernel_ms", "dcp_gpu_db_calibrate_forward", "dcp_exp_sf",
                 "dcp_scores_evalues"):
        assert name in dcp.ABI_SYMBOLS


def test_exp_tail_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_exp_tail.c with the host model alone (no device code) under ASan + UBSan, as a program of its
    own."""
    obj, exe = str(tmp_path / "asan_exp_tail.o"), str(tmp_path / "asan_exp_tail")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_exp_tail.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_exp_tail ok" in r.stdout
