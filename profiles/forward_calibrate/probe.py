"""What a Forward calibration costs, whether the dense scan keeps the pair list's speed, and which law describes the
tail of Forward scores better (profiles/forward_calibrate/probe.txt).  Measured, not gated.

One MI355X, one process, a float DB.  The C3 database (20 000 sampled profiles of the C3 core sizes) against n random
sequences of `len` bases, uniform composition, multi-hit; tail count k.

1. Calibration cost: calibrate_forward(n, len, seed, k) by the host clock, its dense scan by
   forward_dense_kernel_ms (HIP events around all its launches), its two fit kernels by exp_tail_kernel_ms.
2. The dense scan against the parent commit's library (--parent-lib: libdcp_hip.so built from the parent commit, loaded
   beside this one) running forward_pairs on the same full q-major list of the same batch: alternating, one warm-up and
   three runs each; kernel time by events and the whole call by the host clock (the list's arrays are made once, outside
   the clock; the dense call is timed alone and with forward_scores() behind it, since forward_pairs also copies the
   scores out).  The matrices must be the list's bits.
3. The laws: on the fetched Forward scores, per profile, the Kolmogorov distance restricted to the scores >= tau -- the
   empirical distribution of those k_eff scores against the fitted law conditioned on x >= tau -- of the exponential
   tail fit, G(x) = 1 - exp(-lambda (x - tau)), and of gumbel_fit_tail for the same k, G(x) = (F(x) - F(tau)) / (1 -
   F(tau)), F(x) = exp(-exp(-lambda (x - mu))), as profiles/calibrate_tail/probe.py does; the 5 % critical value for m
   points is taken as 1.358 / (sqrt(m) + 0.12 + 0.11 / sqrt(m)), the value for a law given in advance.

    python profiles/forward_calibrate/probe.py [--nprof N] [--nseqs N] [--len L] [--k K] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes as C
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


def load_parent(dcp, path):
    """the parent's library with this one's signatures for the symbols both have"""
    lib = C.CDLL(path)
    for name in dcp.ABI_SYMBOLS:
        if hasattr(lib, name):
            mine = getattr(dcp.lib, name)
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = mine.restype, mine.argtypes
    return lib


def tail_distance(xs, G, k_eff):
    """xs [n, m] scores sorted descending along axis 0, G the conditioned law evaluated on them, k_eff [m]: D per
    profile over its k_eff largest scores"""
    n = xs.shape[0]
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
    ap.add_argument("--nseqs", type=int, default=200)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_calibrate", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda ts: "  ".join(f"{v:.2f}" for v in ts) + f"   median {statistics.median(ts):.2f}"
    sizes = np.asarray(bench.core_sizes_for("c3", args.nprof))
    profs = sample_profiles(dcp, sizes)
    n, L, k, seed = args.nseqs, args.len, args.k, 2025
    gcell = float(sizes.sum()) * n * L / 1e9
    say(f"{len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())}), float DB, x {n} random sequences of {L} bases, uniform,"
        f" multi-hit, seed {seed}: {n * len(profs)} pairs, {gcell:.1f} Gcell; tail count k = {k}")
    sc = dcp.Scanner(0)
    sc.upload_db(profs)

    # 1. the calibration
    call, scan, sel, fit = [], [], [], []
    for it in range(3):
        t0 = time.perf_counter()
        mu, lam, st, tau, k_eff = sc.calibrate_forward(n, L, seed, k)
        t1 = time.perf_counter()
        if it:
            call.append(1e3 * (t1 - t0)), scan.append(sc.forward_dense_kernel_ms())
            sel.append(sc.exp_tail_kernel_ms(0)), fit.append(sc.exp_tail_kernel_ms(1))
    say("1. calibrate_forward, one warm-up and two runs")
    say(f"  the call, ms, host clock:                      {fmt(call)}")
    say(f"  the dense scan's launches, ms, HIP events:     {fmt(scan)}   ({gcell / statistics.median(scan) * 1e3:.2f} Gcell/s)")
    say(f"  tail_select_kernel<double>, ms, HIP events:    {fmt(sel)}")
    say(f"  exp_tail_fit_kernel<double>, ms, HIP events:   {fmt(fit)}")
    names = {dcp.FIT_OK: "OK", dcp.FIT_FLAT: "FLAT", dcp.FIT_NONFINITE: "NONFINITE", dcp.FIT_DIVERGED: "DIVERGED"}
    say("  statuses: " + ", ".join(f"{names[int(s)]} {int((st == s).sum())}" for s in np.unique(st)))
    null, alt = sc.forward_scores()

    # 2. against the parent's forward_pairs on the same list
    if args.parent_lib:
        old = dcp.Scanner(0, lib=load_parent(dcp, args.parent_lib))
        old.upload_db(profs)
        old.random_seqs(n, L, seed)
        sq = np.arange(n, dtype=np.uint32).repeat(len(profs))
        pr = np.tile(np.arange(len(profs), dtype=np.uint32), n)
        t = {key: [] for key in ("dense kernels", "dense call", "dense call + forward_scores", "parent kernels", "parent call")}
        for it in range(4):
            t0 = time.perf_counter()
            sc.forward_dense()
            t1 = time.perf_counter()
            got = sc.forward_scores()
            t2 = time.perf_counter()
            pn, pa = old.forward_pairs(sq, pr)
            t3 = time.perf_counter()
            if it:
                t["dense kernels"].append(sc.forward_dense_kernel_ms()), t["dense call"].append(1e3 * (t1 - t0))
                t["dense call + forward_scores"].append(1e3 * (t2 - t0))
                t["parent kernels"].append(old.forward_kernel_ms), t["parent call"].append(1e3 * (t3 - t2))
        same = np.array_equal(got[0].reshape(-1).view(np.uint64), pn.view(np.uint64)) and \
            np.array_equal(got[1].reshape(-1).view(np.uint64), pa.view(np.uint64))
        say(f"2. forward_dense against the parent commit's forward_pairs of the full list ({len(sq)} pairs, 12 bytes each),"
            " alternating, one warm-up and three runs, ms")
        for key, ts in t.items():
            say(f"  {key:>28}: {fmt(ts)}   spread {max(ts) - min(ts):.2f}")
        dk, pk = statistics.median(t["dense kernels"]), statistics.median(t["parent kernels"])
        say(f"  kernels: dense - parent = {dk - pk:+.2f} ms ({100.0 * (dk - pk) / pk:+.2f} %), the parent's three runs span"
            f" {max(t['parent kernels']) - min(t['parent kernels']):.2f} ms")
        say(f"  the matrices against the parent's list: {'the same bits' if same else 'DIFFERENT BITS'}")
        old.close()
    else:
        say("2. no --parent-lib given: the comparison with the parent commit's forward_pairs was not run")

    # 3. the laws
    with np.errstate(invalid="ignore"):
        x = alt - null
    xs = -np.sort(-x, axis=0)  # descending
    g = [dcp.gumbel_fit_tail(x[:, p], k) for p in range(x.shape[1])]
    gmu, glam, gst = np.array([f[0] for f in g]), np.array([f[1] for f in g]), np.array([f[2] for f in g])
    ok = (st == dcp.FIT_OK) & (gst == dcp.FIT_OK)
    say(f"3. the laws over the scores >= tau, k = {k}: exponential OK {int((st == dcp.FIT_OK).sum())}, gumbel_fit_tail OK"
        f" {int((gst == dcp.FIT_OK).sum())}, both {int(ok.sum())} of {len(profs)} profiles")
    say(f"  exponential: lambda min {lam[ok].min():.4f}  median {np.median(lam[ok]):.4f}  max {lam[ok].max():.4f};"
        f"  mu min {mu[ok].min():.2f}  median {np.median(mu[ok]):.2f}  max {mu[ok].max():.2f};"
        f"  k_eff min {int(k_eff[ok].min())}  max {int(k_eff[ok].max())}")
    say(f"  Gumbel tail: lambda min {glam[ok].min():.4f}  median {np.median(glam[ok]):.4f}  max {glam[ok].max():.4f}")
    De, Dg = [], []
    for c in range(0, len(profs), 2000):
        s = slice(c, c + 2000)
        o = ok[s]
        v, t_, ke = xs[:, s][:, o], tau[s][o], k_eff[s][o]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            Ge = -np.expm1(-lam[s][o][None, :] * (v - t_[None, :]))
            F = lambda w: np.exp(-np.exp(-glam[s][o][None, :] * (w - gmu[s][o][None, :])))
            Ft = F(t_[None, :])
            Gg = (F(v) - Ft) / (1.0 - Ft)
        De.append(tail_distance(v, Ge, ke)), Dg.append(tail_distance(v, Gg, ke))
    De, Dg = np.concatenate(De), np.concatenate(Dg)
    crit = critical(k_eff[ok])
    say(f"  Kolmogorov distance, {len(De)} profiles, 5 % critical value {crit.min():.4f} .. {crit.max():.4f}:")
    say(f"    exponential tail: min {De.min():.4f}  median {np.median(De):.4f}  max {De.max():.4f};  above the critical value"
        f" {100.0 * (De > crit).mean():.1f} %")
    say(f"    Gumbel tail fit:  min {Dg.min():.4f}  median {np.median(Dg):.4f}  max {Dg.max():.4f};  above the critical value"
        f" {100.0 * (Dg > crit).mean():.1f} %")
    say(f"    the exponential law is the closer of the two for {100.0 * (De < Dg).mean():.1f} % of the profiles")
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
