"""What a calibration costs and how well a Gumbel describes the scores (profiles/calibrate/probe.txt).
Measured, not gated.

The C3 database (20 000 sampled profiles of the C3 core sizes) against 1 000 random sequences of 1 kbp, uniform
composition, multi-hit.  One warm-up and three timed runs of the three steps of Scanner.calibrate done by hand: the
generator's kernel and the fit's kernel alone between HIP events on the context's stream (calib_kernel_ms), the scan by
its own events (last_scan_ms), each call by the host clock.  Then, per profile with an OK fit, the Kolmogorov distance
between the 1 000 scores and their fit, D = max_i max(|F(x_(i)) - i / n|, |F(x_(i)) - (i - 1) / n|) with F(x) =
exp(-exp(-lambda (x - mu))), as a histogram (a sample of 1 000 from F itself has D above 0.043 one time in twenty).

    python profiles/calibrate/probe.py [--nprof N] [--nseqs N] [--len L] [--out FILE]
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


def kolmogorov(x, mu, lam):
    """x [n, nprof] scores, mu / lam [nprof]: D per profile"""
    n = x.shape[0]
    F = np.exp(-np.exp(-lam[None, :] * (np.sort(x, axis=0) - mu[None, :])))
    i = np.arange(1, n + 1, dtype=np.float64)[:, None]
    return np.maximum(np.abs(F - i / n), np.abs(F - (i - 1) / n)).max(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--nseqs", type=int, default=1000)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate", "probe.txt"))
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
    say(f"{len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())}) x {args.nseqs} random sequences of {args.len} bases,"
        f" uniform, multi-hit, seed 2024")
    t = {k: [] for k in ("gen_call", "gen_kernel", "scan_call", "scan_events", "fit_call", "fit_kernel")}
    fit = None
    for it in range(4):  # the first is the warm-up
        t0 = time.perf_counter()
        sc.random_seqs(args.nseqs, args.len, 2024)
        t1 = time.perf_counter()
        sc.scan(True, False, float("inf"), keep_scores=True)
        t2 = time.perf_counter()
        fit = sc.fit_gumbel()
        t3 = time.perf_counter()
        if it:
            for k, v in (("gen_call", 1e3 * (t1 - t0)), ("gen_kernel", sc.calib_kernel_ms(0)), ("scan_call", 1e3 * (t2 - t1)),
                         ("scan_events", sc.last_scan_ms), ("fit_call", 1e3 * (t3 - t2)), ("fit_kernel", sc.calib_kernel_ms(1))):
                t[k].append(v)
    fmt = lambda ts: "  ".join(f"{v:.4f}" for v in ts) + f"   median {statistics.median(ts):.4f}"
    say(f"  random_seqs   ms, the call:                    {fmt(t['gen_call'])}")
    say(f"  random_words_kernel ms, HIP events:            {fmt(t['gen_kernel'])}")
    say(f"  scan          ms, the call (kernel {sc.last_scan_kernel}):         {fmt(t['scan_call'])}")
    say(f"  scan          ms, its own events:              {fmt(t['scan_events'])}"
        f"   = {sc.cells / (1e6 * statistics.median(t['scan_events'])):.0f} Gcell/s")
    say(f"  fit_gumbel    ms, the call:                    {fmt(t['fit_call'])}")
    say(f"  gumbel_fit_kernel ms, HIP events:              {fmt(t['fit_kernel'])}")
    mu, lam, st = fit
    names = {dcp.FIT_OK: "OK", dcp.FIT_FLAT: "FLAT", dcp.FIT_NONFINITE: "NONFINITE", dcp.FIT_DIVERGED: "DIVERGED"}
    say("  statuses: " + ", ".join(f"{names[int(s)]} {int((st == s).sum())}" for s in np.unique(st)))
    ok = st == dcp.FIT_OK
    say(f"  lambda: min {lam[ok].min():.4f}  median {np.median(lam[ok]):.4f}  max {lam[ok].max():.4f};"
        f"  mu: min {mu[ok].min():.2f}  median {np.median(mu[ok]):.2f}  max {mu[ok].max():.2f}")
    null, alt = sc.scores()
    x = alt.astype(np.float64) - null.astype(np.float64)
    D = np.concatenate([kolmogorov(x[:, c:c + 2000][:, ok[c:c + 2000]], mu[c:c + 2000][ok[c:c + 2000]], lam[c:c + 2000][ok[c:c + 2000]])
                        for c in range(0, len(profs), 2000)])
    say(f"  Kolmogorov distance of {args.nseqs} scores from their fit, {len(D)} profiles: min {D.min():.4f}  median {np.median(D):.4f}"
        f"  max {D.max():.4f}")
    edges = [0.0, 0.01, 0.02, 0.03, 0.043, 0.06, 0.08, 0.1, 0.15, 0.2, 0.3, 1.0]
    counts, _ = np.histogram(D, edges)
    for lo, hi, c in zip(edges[:-1], edges[1:], counts):
        say(f"    [{lo:.3f}, {hi:.3f})  {int(c):6d}  {'#' * int(round(60.0 * c / max(1, counts.max())))}")
    msizes = sizes[ok]
    for lo, hi in ((1, 33), (33, 129), (129, 513), (513, 1 << 30)):
        sel = (msizes >= lo) & (msizes < hi)
        if sel.any():
            say(f"    core size {lo}..{min(hi, int(sizes.max()) + 1) - 1}: {int(sel.sum())} profiles, median D {np.median(D[sel]):.4f}")
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
