"""The Gumbel fit and E-values: dcp_gumbel_fit / dcp_gumbel_sf / dcp_hits_evalues on the host (csrc/dcp_model.cpp) and
gumbel_fit_kernel (csrc/dcp_calib.hip) behind dcp_gpu_fit_gumbel / dcp_gpu_db_calibrate on the device.  The rule is
csrc/dcp_calib.h: double arithmetic, every sum in index order, exactly 12 Newton steps.

The bound.  Two evaluations of the rule differ in exp, log and sqrt only (a few units in the last place each).  The sums
have non-negative terms in the same order: each carries at most about (N + 8) 2^-53 relative error.  f is that error
times 1 / lambda, |df| >= 1 / lambda^2, and Newton's fixed point moves by f / df: about (N + 8) 2^-53 relative, 2^-45 for
N = 200.  The tests allow |d lambda| <= 2^-32 lambda and |d mu| <= 2^-32 (|mu| + 1 / lambda), a factor of several thousand
over that, and print the maxima they saw.

CPU: the host twin against a numpy restatement on the oracle's scores of generator sequences; the statuses; a stride;
     the tail function; E-values; tests/c/asan_calib.c under ASan + UBSan as a program of its own.
GPU: the device fit against the host twin on scores() of the same scan at the lane edges; FLAT and NONFINITE lanes;
     calibrate() against its three steps; the refusals; E-values of a planted gene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, hit_fields
from test_c_host import ROOT
from test_gpu_parity import pfam_like_params, planted_query

PRECISIONS = (32, 64)
REL = 2.0 ** -32
FIT_M = (3, 8, 40, 64, 65, 130, 513)
FIT_SEEDS = (7, 8, 9)
FIT_SHAPES = ((8, 30), (16, 30), (32, 45), (64, 60), (300, 33))


def seqsum(v):
    return np.cumsum(v)[-1]  # strictly sequential, in index order


def np_fit(x, trace=None):
    """the rule as stated: (mu, lambda, status) with status as the module's FIT_* values"""
    x = np.asarray(x, np.float64)
    n = len(x)
    if not np.isfinite(x).all():
        return np.nan, np.nan, 17
    with np.errstate(all="ignore"):
        m, mean = x.min(), seqsum(x) / n
        var = seqsum((x - mean) * (x - mean)) / (n - 1)
        if var == 0:
            return np.nan, np.nan, 16
        lam = np.pi / np.sqrt(6.0 * var)
        y = x - m
        diverged, settled = False, False
        for _ in range(12):
            w = np.exp(-(lam * y))
            s0, s1, s2 = seqsum(w), seqsum(y * w), seqsum((y * y) * w)
            r = s1 / s0
            f = 1.0 / lam - (mean - m) + r
            df = -1.0 / (lam * lam) - s2 / s0 + r * r
            nxt = lam - f / df
            if not np.isfinite(nxt) or not nxt > 0:
                diverged, nxt = True, lam
            settled = abs(nxt - lam) <= 2.0 ** -40 * nxt
            if trace is not None:
                trace.append(abs(nxt - lam) / nxt)
            lam = nxt
        if diverged or not settled:
            return np.nan, np.nan, 18
        return m - np.log(seqsum(np.exp(-(lam * y))) / n) / lam, lam, 0


def within_bound(got, want):
    """(ok, relative deviation of lambda, deviation of mu in units of |mu| + 1 / lambda)"""
    (gm, gl), (wm, wl) = got, want
    dl, dm = abs(gl - wl) / wl, abs(gm - wm) / (abs(wm) + 1.0 / wl)
    return dl <= REL and dm <= REL, dl, dm


# ---- CPU: the twin against the restatement -----------------------------------------------------------------------

_ORACLE_SCORES, _ORACLE_PROFS = {}, {}


def oracle_scores(dcp, oracle, precision, seed, shape):
    """x[q][p] = alt - null in double of the oracle's scan of generator sequences against sample(100 + M, M)"""
    key = (precision, seed, shape)
    if key not in _ORACLE_SCORES:
        if precision not in _ORACLE_PROFS:
            _ORACLE_PROFS[precision] = [oracle.sample(100 + M, M, ENTRY_DIST_OCCUPANCY, 0.01) for M in FIT_M]
        oprofs = _ORACLE_PROFS[precision]
        n, L = shape
        seqs = [bytes(dcp.random_seq(seed, q, L)) for q in range(n)]
        _, on, oa, _, _ = oracle.scan_resident(oprofs, seqs, True, False, 10.0, 4)  # the bits of scan(), tables built once
        _ORACLE_SCORES[key] = oa.astype(np.float64) - on.astype(np.float64)
    return _ORACLE_SCORES[key]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_twin_equals_the_restatement_on_oracle_scores(dcp, oracle32, oracle64, precision):
    oracle = oracle64 if precision == 64 else oracle32
    worst_l = worst_m = 0.0
    slowest = 0
    for seed in FIT_SEEDS:
        for shape in FIT_SHAPES:
            x = oracle_scores(dcp, oracle, precision, seed, shape)
            assert x.shape == (shape[0], len(FIT_M)) and np.isfinite(x).all()
            for p in range(len(FIT_M)):
                where = (precision, seed, shape, FIT_M[p])
                steps = []
                wm, wl, ws = np_fit(x[:, p], steps)
                # the premise: the restatement converges with room to spare -- a relative step below 1e-14 after at
                # most 8 of the 12 steps (quadratic convergence: the steps behind it change nothing)
                assert ws == dcp.FIT_OK and wl > 0 and min(steps[:8]) < 1e-14, (where, steps)
                slowest = max(slowest, 1 + next(i for i, d in enumerate(steps) if d < 1e-14))
                gm, gl, gs = dcp.gumbel_fit(x[:, p])  # a column: stride len(FIT_M)
                assert gs == dcp.FIT_OK, where
                ok, dl, dm = within_bound((gm, gl), (wm, wl))
                assert ok, (where, dl, dm)
                assert (gm, gl, gs) == dcp.gumbel_fit(np.ascontiguousarray(x[:, p])), where
                worst_l, worst_m = max(worst_l, dl), max(worst_m, dm)
    print("precision %d: twin vs restatement, max |d lambda| / lambda = %.3g, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % (precision, worst_l, worst_m))
    print("precision %d: the slowest fit took %d of the 12 steps to a relative step below 1e-14" % (precision, slowest))


def test_statuses_and_strides(dcp):
    rng = np.random.default_rng(17)
    x = rng.gumbel(-3.0, 2.5, 400)
    mu, lam, st = dcp.gumbel_fit(x)
    assert st == dcp.FIT_OK and abs(lam - 0.4) < 0.05 and abs(mu + 3.0) < 0.5
    assert within_bound((mu, lam), np_fit(x)[:2])[0]
    # flat
    for flat in (np.zeros(5), np.full(2, -7.25), np.full(8, 3.75)):  # counts whose mean is the value itself
        mu, lam, st = dcp.gumbel_fit(flat)
        assert st == dcp.FIT_FLAT == np_fit(flat)[2] and np.isnan(mu) and np.isnan(lam)
    # one non-finite value, anywhere
    for bad in (-np.inf, np.inf, np.nan):
        for at in (0, 200, 399):
            y = x.copy()
            y[at] = bad
            mu, lam, st = dcp.gumbel_fit(y)
            assert st == dcp.FIT_NONFINITE == np_fit(y)[2] and np.isnan(mu) and np.isnan(lam), (bad, at)
    # n < 2
    for n in (0, 1):
        with pytest.raises(dcp.DcpError) as e:
            dcp.gumbel_fit(x[:n])
        assert e.value.rc == dcp.RC_EINVAL
    mu_c, lam_c = C.c_double(5.0), C.c_double(6.0)
    for args in ((x.ctypes.data, 1, 1), (None, 10, 1), (x.ctypes.data, 10, 0)):
        assert dcp.lib.dcp_gumbel_fit(*args, C.byref(mu_c), C.byref(lam_c)) == dcp.RC_EINVAL
    assert dcp.lib.dcp_gumbel_fit(x.ctypes.data, 10, 1, None, C.byref(lam_c)) == dcp.RC_EINVAL
    assert (mu_c.value, lam_c.value) == (5.0, 6.0)
    assert dcp.gumbel_fit(x[:2])[2] == dcp.FIT_OK == np_fit(x[:2])[2]
    # strides: every third value, and a column of a matrix
    assert dcp.gumbel_fit(x[::3]) == dcp.gumbel_fit(x[::3].copy())
    mat = rng.gumbel(0.0, 1.0, (50, 7))
    for p in range(7):
        assert dcp.gumbel_fit(mat[:, p]) == dcp.gumbel_fit(mat[:, p].copy())
    # a variance that overflows: lambda starts at 0 and no step leaves it finite and positive
    for wild in (np.array([0.0, 1e200, 3e200]), np.array([-1e308, 1e308])):
        mu, lam, st = dcp.gumbel_fit(wild)
        assert st == dcp.FIT_DIVERGED == np_fit(wild)[2] and np.isnan(mu) and np.isnan(lam)


def test_tail_function(dcp):
    for mu, lam in ((0.0, 1.0), (-12.5, 0.31), (40.0, 0.693), (3.0, 2.5)):
        for s in (mu, mu - 10.0 / lam, mu + 10.0 / lam, mu + 40.0 / lam, mu + 300.0 / lam, mu + 700.0 / lam):
            want = -np.expm1(-np.exp(-lam * (s - mu)))
            got = dcp.gumbel_sf(mu, lam, s)
            assert abs(got - want) <= 1e-12 * want, (mu, lam, s, got, want)
        # far in the tail the probability is exp(-lambda (s - mu)) itself: 1 - exp(-t) would have lost it below 1e-16
        for z in (40.0, 300.0, 700.0):
            got = dcp.gumbel_sf(mu, lam, mu + z / lam)
            assert got > 0 and abs(got - np.exp(-z)) <= 1e-12 * np.exp(-z), (mu, lam, z)
        assert dcp.gumbel_sf(mu, lam, mu - 10.0 / lam) == 1.0


def test_hit_evalues(dcp):
    mu, lam = np.array([1.0, 2.0, 3.0]), np.array([0.5, 0.6, 0.7])
    status = np.array([dcp.FIT_OK, dcp.FIT_NONFINITE, dcp.FIT_OK], np.uint8)
    for dtype in (dcp.HIT_DTYPE, dcp.HIT64_DTYPE):
        hits = np.zeros(4, dtype)
        hits["seq_idx"] = [0, 1, 2, 3]
        hits["profile_idx"] = [0, 1, 2, 0]
        hits["null_loglik"] = [-100.0, -90.0, -80.0, -70.5]
        hits["alt_loglik"] = [-90.0, -85.0, -50.0, -71.0]
        e = dcp.hit_evalues(hits, mu, lam, status, 1000.0)
        s = hits["alt_loglik"].astype(np.float64) - hits["null_loglik"].astype(np.float64)
        want = 1000.0 * -np.expm1(-np.exp(-lam[hits["profile_idx"]] * (s - mu[hits["profile_idx"]])))
        assert np.isnan(e[1]) and np.allclose(e[[0, 2, 3]], want[[0, 2, 3]], rtol=1e-12, atol=0)
        assert (dcp.hit_evalues(hits, mu, lam, status, 0.0)[[0, 2, 3]] == 0).all()
        assert len(dcp.hit_evalues(hits[:0], mu, lam, status, 5.0)) == 0
        for st in (dcp.FIT_FLAT, dcp.FIT_DIVERGED):
            assert np.isnan(dcp.hit_evalues(hits, mu, lam, np.full(3, st, np.uint8), 1.0)).all()
        # the refusals: nothing written
        fn = dcp.lib.dcp_hits_evalues64 if dtype == dcp.HIT64_DTYPE else dcp.lib.dcp_hits_evalues
        out = np.full(4, 9.0)
        ptr = lambda a: a.ctypes.data
        assert fn(ptr(hits), 4, ptr(mu), ptr(lam), ptr(status), 2, 1000.0, ptr(out)) == dcp.RC_EINVAL  # profile 2 >= 2
        for bad in (np.nan, np.inf, -1.0):
            assert fn(ptr(hits), 4, ptr(mu), ptr(lam), ptr(status), 3, bad, ptr(out)) == dcp.RC_EINVAL
        for k in range(5):
            args = [ptr(hits), ptr(mu), ptr(lam), ptr(status), ptr(out)]
            args[k] = None
            assert fn(args[0], 4, args[1], args[2], args[3], 3, 1000.0, args[4]) == dcp.RC_EINVAL
        assert (out == 9.0).all()
        with pytest.raises(dcp.DcpError):
            dcp.hit_evalues(hits, mu[:2], lam[:2], status[:2], 1000.0)
        with pytest.raises(dcp.DcpError):
            dcp.hit_evalues(hits, mu, lam, status, -1.0)


def test_calib_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_calib.c with the host model alone (no device code) under ASan + UBSan, as a program of its own."""
    obj, exe = str(tmp_path / "asan_calib.o"), str(tmp_path / "asan_calib")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_calib.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_calib ok" in r.stdout


# ---- GPU: the device fit against the host twin -------------------------------------------------------------------

LANE_M = (3, 8, 17, 40, 64, 65, 100, 130)  # core sizes, cycled
LANE_NPROF = (1, 63, 64, 65, 130)           # the edges of a 64-lane block
LANE_N = (2, 3, 64, 200)

_LANE_PROFS = {}


def lane_profiles(dcp, precision, n):
    if precision not in _LANE_PROFS:
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
        _LANE_PROFS[precision] = [dcp.ProteinProfile.sample(700 + i, LANE_M[i % len(LANE_M)], cfg, f"L{i:03d}", precision=precision)
                                  for i in range(max(LANE_NPROF))]
    return _LANE_PROFS[precision][:n]


def host_fits(dcp, sc):
    """the host twin on scores() of the scan that is resident: (mu, lam, status) arrays"""
    null, alt = sc.scores()
    with np.errstate(invalid="ignore"):  # -inf - -inf of an epsilon = 0 lane
        x = alt.astype(np.float64) - null.astype(np.float64)
    fits = [dcp.gumbel_fit(x[:, p]) for p in range(x.shape[1])]
    return (np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[2] for f in fits], np.uint8))


def compare_fits(got, want, where):
    """statuses equal, NaN where not OK, lambda and mu within the bound: the two maxima"""
    (gm, gl, gs), (wm, wl, ws) = got, want
    assert gs.dtype == np.uint8 and np.array_equal(gs, ws), (where, gs, ws)
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
def test_device_fit_equals_the_host_twin(dcp, precision, nprof):
    sc = dcp.Scanner(0)
    sc.upload_db(lane_profiles(dcp, precision, nprof))
    worst = (0.0, 0.0)
    for n in LANE_N:
        sc.random_seqs(n, 100, 40 + n)
        sc.scan(True, False, 10.0)
        got = sc.fit_gumbel()
        want = host_fits(dcp, sc)
        # (a 3-node profile's 64 scores lean left, and the first Newton step from the moment estimate leaves lambda > 0:
        # DIVERGED on both sides.  Most lanes must be OK for the bound to be looked at.)
        if n == 200 and nprof >= 63:
            assert (want[2] == dcp.FIT_OK).sum() >= 0.9 * nprof, (precision, nprof, n, want[2])
        worst = tuple(max(a, b) for a, b in zip(worst, compare_fits(got, want, (precision, nprof, n))))
        assert np.array_equal(bits(got[0]), bits(sc.fit_gumbel()[0]))  # the scan's results stay valid
    print("precision %d, %d profiles: device vs host twin, max |d lambda| / lambda = %.3g, max |d mu| / (|mu| + 1 / lambda) = %.3g"
          % ((precision, nprof) + worst))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_flat_and_nonfinite_lanes(dcp, precision):
    profs = lane_profiles(dcp, precision, 70)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    # two identical sequences: no variance in any lane
    s = dcp.random_seq(3, 0, 100)
    sc.upload_seqs([s, s])
    sc.scan(True, False, 10.0)
    mu, lam, st = sc.fit_gumbel()
    assert (st == dcp.FIT_FLAT).all() and np.isnan(mu).all() and np.isnan(lam).all()
    # one epsilon = 0 profile among the others: its lane alone is NONFINITE, the others keep their bits
    at = 37
    sc.random_seqs(64, 100, 5)
    sc.scan(True, False, 10.0)
    base = sc.fit_gumbel()
    assert (base[2] == dcp.FIT_OK).sum() >= 60 and base[2][at - 1] == base[2][at] == dcp.FIT_OK
    zero = dcp.ProteinProfile.sample(999, 40, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    sc.upload_db(profs[:at] + [zero] + profs[at:])
    sc.random_seqs(64, 100, 5)
    sc.scan(True, False, 10.0)
    null, alt = sc.scores()
    assert not (np.isfinite(alt[:, at]) & np.isfinite(null[:, at])).all()
    mu, lam, st = sc.fit_gumbel()
    assert st[at] == dcp.FIT_NONFINITE and np.isnan(mu[at]) and np.isnan(lam[at])
    rest = np.arange(len(profs) + 1) != at
    assert np.array_equal(st[rest], base[2])
    assert np.array_equal(bits(mu[rest]), bits(base[0])) and np.array_equal(bits(lam[rest]), bits(base[1]))
    compare_fits((mu, lam, st), host_fits(dcp, sc), precision)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,kernel", [(32, 0), (32, 1), (32, 2), (32, 3), (64, 0), (64, 1), (64, 4)])
def test_calibrate_is_its_three_steps(dcp, precision, kernel):
    profs = lane_profiles(dcp, precision, 65)
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    n, L, seed, probs = 80, 90, 77, (0.3, 0.2, 0.2, 0.3)
    a._check(a._lib.dcp_gpu_set_lrt_threshold64(a._c, -1e300))  # a double DB's own threshold: restored behind the scan
    got = a.calibrate(n, L, seed, probs, multi_hits=True, hmmer3_compat=False, kernel=kernel)
    b.random_seqs(n, L, seed, probs)
    b.scan(True, False, float("inf"), keep_scores=True, kernel=kernel)
    want = b.fit_gumbel()
    for x, y in zip(got, want):
        assert np.array_equal(bits(x.astype(np.float64)), bits(y.astype(np.float64))), (precision, kernel)
    assert (got[2] == dcp.FIT_OK).sum() >= 0.9 * len(profs), got[2]
    # what it leaves: the random batch and that scan
    assert (a.nseqs, a.strands, a.windows) == (n, 1, None) and a.last_scan_kernel == b.last_scan_kernel
    for q in (0, 1, n - 1):
        assert np.array_equal(a.fetch_seq(q), dcp.random_seq(seed, q, L, probs))
    for x, y in zip(a.scores(), b.scores()):
        assert np.array_equal(bits(x), bits(y))
    assert len(a.hits()) == 0 and len(b.hits()) == 0
    for x, y in zip(a.fit_gumbel(), got):
        assert np.array_equal(bits(x.astype(np.float64)), bits(y.astype(np.float64)))
    if precision == 64:  # the caller's threshold is in force again: a raw scan reports every finite pair
        prm = dcp.ScanParams(1, 0, float("inf"), 1, 1)
        a._check(a._lib.dcp_gpu_scan(a._c, C.byref(prm)))
        a.sync()
        assert len(a.hits()) == n * len(profs)
    # a bad argument is the generator's refusal, and the batch stays
    with pytest.raises(dcp.DcpError) as e:
        a.calibrate(0, L, seed)
    assert e.value.rc == dcp.RC_EINVAL and a.nseqs == n
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_of_the_fit(dcp, precision):
    profs = lane_profiles(dcp, precision, 10)
    rng = np.random.default_rng(precision)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(40, 200, 12)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    mu, lam, st = np.full(10, 9.0), np.full(10, 9.0), np.full(10, 9, np.uint8)
    ptr = lambda a: a.ctypes.data

    def refused(*words):
        assert sc._lib.dcp_gpu_fit_gumbel(sc._c, ptr(mu), ptr(lam), ptr(st)) == dcp.RC_EINVAL
        msg = sc._lib.dcp_gpu_last_error(sc._c).decode()
        assert all(w in msg for w in words), msg
        assert (mu == 9.0).all() and (lam == 9.0).all() and (st == 9).all()

    refused("no scan")
    sc.scan(True, False, 10.0, keep_scores=True)
    want = [bits(x).copy() for x in sc.scores()]
    want_hits = hit_fields(sc.hits())
    ok = sc.fit_gumbel()
    assert (ok[2] == dcp.FIT_OK).any()
    for k in range(3):
        args = [ptr(mu), ptr(lam), ptr(st)]
        args[k] = None
        assert sc._lib.dcp_gpu_fit_gumbel(sc._c, *args) == dcp.RC_EINVAL
    sc.scan(True, False, 10.0, keep_scores=False)
    refused("dense scores")
    sc.scan_pairs([0, 1], [1, 2])
    refused("dense scores")
    sc.scan(True, False, 10.0, q_range=(0, 11))
    refused("whole batch")
    sc.scan(True, False, 10.0, q_range=(1, 12))
    refused("whole batch")
    sc.upload_seqs(seqs[:1])
    refused("no scan")
    sc.scan(True, False, 10.0)
    refused("2 sequences")
    # a normal scan behind a calibration is what it was
    sc.calibrate(50, 60, 1)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0, keep_scores=True)
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    assert hit_fields(sc.hits()) == want_hits
    for x, y in zip(sc.fit_gumbel(), ok):
        assert np.array_equal(bits(x.astype(np.float64)), bits(y.astype(np.float64)))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_evalues_of_a_planted_gene(dcp, oracle32, oracle64, precision):
    """The hits of a planted gene among random sequences: E-values against numpy.  Printed, not gated: the planted
    pair's E-value beside the smallest one among the random sequences (nsearched = the batch size)."""
    oracle = oracle64 if precision == 64 else oracle32
    rng = np.random.default_rng(8100 + precision)
    sizes = (40, 130)
    params = [pfam_like_params(rng, M) for M in sizes]
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
    profs = [dcp.ProteinProfile.from_params(*prm, cfg, f"EV{i}", precision=precision) for i, prm in enumerate(params)]
    oprofs = [oracle.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01) for prm in params]
    L, n = 600, 200
    gene = planted_query(rng, oprofs[1], sizes[1], flank=12)
    assert len(gene) <= L
    seqs = [dcp.random_seq(4242, q, L) for q in range(n)]
    seqs[0] = seqs[0].copy()
    seqs[0][50:50 + len(gene)] = gene[:L - 50]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    mu, lam, st = sc.calibrate(n, L, 99)
    assert (st == dcp.FIT_OK).all()
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e30)
    hits = sc.hits()
    assert len(hits) == n * len(profs)
    ev = dcp.hit_evalues(hits, mu, lam, st, float(n))
    p = hits["profile_idx"]
    s = hits["alt_loglik"].astype(np.float64) - hits["null_loglik"].astype(np.float64)
    want = n * -np.expm1(-np.exp(-lam[p] * (s - mu[p])))
    assert np.allclose(ev, want, rtol=1e-12, atol=0)
    planted = (hits["seq_idx"] == 0) & (p == 1)
    print("precision %d: planted pair E = %.3g (score %.1f); smallest E among %d random pairs = %.3g"
          % (precision, ev[planted][0], s[planted][0], (~planted).sum(), ev[~planted].min()))
    sc.close()
