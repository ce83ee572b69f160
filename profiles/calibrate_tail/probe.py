"""What the tail fit costs and whether it describes the scores' tail better than the whole-sample fit
(profiles/calibrate_tail/probe.txt).  Measured, not gated.

The setting of profiles/calibrate/probe.py: the C3 database (20 000 sampled profiles of the C3 core sizes) against 1 000
random sequences of 1 kbp, uniform composition, multi-hit, one scan.  On that scan's dense scores, one warm-up and
three timed runs each of fit_gumbel() and of fit_gumbel_tail(k), k = 1 000, 500, 250, 100: the kernels alone between HIP
events on the context's stream (calib_kernel_ms, calib_tail_kernel_ms), each call by the host clock.  Then, per k and
per profile with an OK fit, the Kolmogorov distance restricted to the scores >= tau: the empirical distribution of
those k_eff scores against the fitted law conditioned on x >= tau, G(x) = (F(x) - F(tau)) / (1 - F(tau)), F(x) =
exp(-exp(-lambda (x - mu))); D = max_i max(|G(x_(i)) - i / k_eff|, |G(x_(i)) - (i - 1) / k_eff|).  Beside it the same
distance, over the same scores, of the whole-sample fit.  The 5 % critical value for m points is taken as 1.358 /
(sqrt(m) + 0.12 + 0.11 / sqrt(m)); it is the value for a law given in advance, so with two fitted parameters a true
Gumbel tail exceeds it less often than one time in twenty.

    python profiles/calibrate_tail/probe.py [--nprof N] [--nseqs N] [--len L] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import sample_profiles  # noqa: E402


def tail_kolmogorov(xs, mu, lam, tau, k_eff):
    """xs [n, m] scores sorted descending along axis 0; mu / lam / tau / k_eff [m]: D per profile over its k_eff
    largest scores against the law conditioned on x >= tau"""
    n = xs.shape[0]
    F = lambda v: np.exp(-np.exp(-lam[None, :] * (v - mu[None, :])))
    Ft = F(tau[None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        G = (F(xs) - Ft) / (1.0 - Ft)
    j = np.arange(n, dtype=np.float64)[:, None]
    ke = k_eff[None, :].astype(np.float64)
    i = ke - j  # the i-th smallest of the tail sits at descending index k_eff - i
    d = np.maximum(np.abs(G - i / ke), np.abs(G - (i - 1.0) / ke))
    return np.where(j < ke, d, 0.0).max(axis=0)


def critical(m):
    m = np.asarray(m, np.float64)
    return 1.358 / (np.sqrt(m) + 0.12 + 0.11 / np.sqrt(m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--nseqs", type=int, default=1000)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_tail", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = bench.core_sizes_for("c3", args.nprof)
    profs = sample_profiles(dcp, sizes)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    n = args.nseqs
    say(f"{len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())}) x {n} random sequences of {args.len} bases,"
        f" uniform, multi-hit, seed 2024")
    sc.random_seqs(n, args.len, 2024)
    sc.scan(True, False, float("inf"), keep_scores=True)
    say(f"  scan          ms, its own events (kernel {sc.last_scan_kernel}):   {sc.last_scan_ms:.4f}")
    fmt = lambda ts: "  ".join(f"{v:.4f}" for v in ts) + f"   median {statistics.median(ts):.4f}"

    def timed(call, kernels):
        """one warm-up and three timed runs: the last result, the calls' ms, and the kernels' ms by events"""
        t = [[] for _ in range(1 + len(kernels))]
        out = None
        for it in range(4):
            t0 = time.perf_counter()
            out = call()
            t1 = time.perf_counter()
            if it:
                t[0].append(1e3 * (t1 - t0))
                for a, ms in enumerate(kernels):
                    t[1 + a].append(ms())
        return out, t

    whole, t = timed(sc.fit_gumbel, [lambda: sc.calib_kernel_ms(1)])
    say(f"  fit_gumbel      ms, the call:                  {fmt(t[0])}")
    say(f"  gumbel_fit_kernel ms, HIP events:              {fmt(t[1])}")
    null, alt = sc.scores()
    xs = -np.sort(-(alt.astype(np.float64) - null.astype(np.float64)), axis=0)  # descending
    names = {dcp.FIT_OK: "OK", dcp.FIT_FLAT: "FLAT", dcp.FIT_NONFINITE: "NONFINITE", dcp.FIT_DIVERGED: "DIVERGED"}
    for k in [k for k in (n, n // 2, n // 4, n // 10) if k >= 2]:
        fit, t = timed(lambda: sc.fit_gumbel_tail(k), [lambda: sc.calib_tail_kernel_ms(0), lambda: sc.calib_tail_kernel_ms(1)])
        mu, lam, st, tau, k_eff = fit
        say(f"k = {k}")
        say(f"  fit_gumbel_tail ms, the call:                  {fmt(t[0])}")
        say(f"  tail_select_kernel ms, HIP events:             {fmt(t[1])}")
        say(f"  gumbel_fit_tail_kernel ms, HIP events:         {fmt(t[2])}")
        say("  statuses: " + ", ".join(f"{names[int(s)]} {int((st == s).sum())}" for s in np.unique(st)))
        ok = (st == dcp.FIT_OK) & (whole[2] == dcp.FIT_OK)
        say(f"  lambda: min {lam[ok].min():.4f}  median {np.median(lam[ok]):.4f}  max {lam[ok].max():.4f};"
            f"  mu: min {mu[ok].min():.2f}  median {np.median(mu[ok]):.2f}  max {mu[ok].max():.2f};"
            f"  k_eff: min {int(k_eff[ok].min())}  max {int(k_eff[ok].max())}")
        assert np.array_equal(tau[ok], xs[k - 1][ok])  # the k-th largest, as numpy sorts it
        if k == n:
            same = np.array_equal(mu[ok].view(np.uint64), whole[0][ok].view(np.uint64)) and \
                np.array_equal(lam[ok].view(np.uint64), whole[1][ok].view(np.uint64)) and np.array_equal(st, whole[2])
            say(f"  k = n against fit_gumbel: {'the same bits' if same else 'DIFFERENT BITS'}")
        Dt, Dw = [], []
        for c in range(0, len(profs), 2000):
            s = slice(c, c + 2000)
            o = ok[s]
            Dt.append(tail_kolmogorov(xs[:, s][:, o], mu[s][o], lam[s][o], tau[s][o], k_eff[s][o]))
            Dw.append(tail_kolmogorov(xs[:, s][:, o], whole[0][s][o], whole[1][s][o], tau[s][o], k_eff[s][o]))
        Dt, Dw = np.concatenate(Dt), np.concatenate(Dw)
        crit = critical(k_eff[ok])
        say(f"  Kolmogorov distance over the scores >= tau, {len(Dt)} profiles, 5 % critical value {crit.min():.4f} .. {crit.max():.4f}:")
        say(f"    tail fit:         min {Dt.min():.4f}  median {np.median(Dt):.4f}  max {Dt.max():.4f};  above the critical value"
            f" {100.0 * (Dt > crit).mean():.1f} %")
        say(f"    whole-sample fit: min {Dw.min():.4f}  median {np.median(Dw):.4f}  max {Dw.max():.4f};  above the critical value"
            f" {100.0 * (Dw > crit).mean():.1f} %")
        say(f"    the tail fit is the closer of the two for {100.0 * (Dt < Dw).mean():.1f} % of the profiles")
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
