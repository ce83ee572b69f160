"""The f64 query-lane kernel (kernel 4) beside the f64 row sweep (kernel 1) of the same build, alternating in one
process, on the C2-sized job of f64_rate_probe.py: 1 000 profiles (bench.py's c2 core sizes, 100..300 nodes) against
64, 256, 1 000 and 4 000 queries of 300 nt, multi-hit and uni-hit, plus mixed-length batches: one of 256 queries of
100 nt .. 10 kbp (which no plan can help: its longest group bounds it) and bench.py's C5 mix (make_queries, log-uniform
100 nt .. 10 kbp) at 1 000 and 2 000 queries, multi-hit, where kernel 4's packed batch plan pays.
Each case: one warm-up scan of each kernel, then `--reps` rounds of (kernel 1, kernel 4), HIP events around a scan's
launches (the redo launches included).  With --other-lib PATH (another build of the library, the parent commit's say)
kernel 4 of that build runs between the two in every round, in a context of its own on the same device.
Prints one JSON line: every time, the best times' Gcell/s, each kernel's spread (max - min of its repeated times: the
noise floor), the redo-pair count, kernel 4's batch plan, and whether the kernels' hit records are equal.
python profiles/f64_qlane_probe.py [--nprof 1000 --qlen 300 --reps 3 --mixed 256 --c5mix 1000 2000 --other-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_product  # noqa: E402


def same_hits(a, b):
    return bool(len(a) == len(b) and a.tobytes() == b.tobytes())


def load_other(dcp, path):
    """Another build of the library with this build's signatures; a symbol it lacks stays unbound."""
    lib = C.CDLL(path)
    for name in dcp.ABI_SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = getattr(dcp.lib, name).restype, getattr(dcp.lib, name).argtypes
    return lib


def consecutive_rows(lens):
    """what a tile cost before the plan: blocks of 256 consecutive queries of the length order, each to its longest"""
    s = np.sort(np.asarray(lens))
    return int(sum(int(s[min(b + 255, len(s) - 1)]) for b in range(0, len(s), 256)))


def run_case(dcp, sc, other, seqs, multi, reps, k1_reps=None):
    sc.upload_seqs(seqs)
    if other:
        other.upload_seqs(seqs)
    K1, K4 = dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE64
    legs = [("k1", sc, K1), ("other_k4", other, K4), ("k4", sc, K4)]
    legs = [leg for leg in legs if leg[1] is not None]
    ms = {name: [] for name, _, _ in legs}
    hits = {}
    redo = 0
    plan = None
    for r in range(reps + 1):
        for name, s, k in legs:
            if name == "k1" and k1_reps is not None and r > k1_reps:
                continue
            s.scan(multi, False, 10.0, keep_scores=False, kernel=k)
            assert s.last_scan_kernel == k
            if r:
                ms[name].append(s.last_scan_ms)
            else:
                hits[name] = s.hits(cap=1 << 22)
                if name == "k4":
                    redo = s.last_scan_redo_pairs
                    plan = s.last_scan_query_plan
    cells = sc.cells
    k1, k4 = ms["k1"], ms["k4"]
    out = {"nq": len(seqs), "multi_hits": bool(multi), "cells": int(cells), "k1_ms": k1, "k4_ms": k4,
           "k1_gcells": cells / (min(k1) * 1e-3) / 1e9, "k4_gcells": cells / (min(k4) * 1e-3) / 1e9,
           "k1_spread_ms": max(k1) - min(k1), "k4_spread_ms": max(k4) - min(k4), "k4_faster_by_ms": min(k1) - min(k4),
           "redo_pairs": int(redo), "hits": int(len(hits["k1"])), "hits_equal": same_hits(hits["k1"], hits["k4"]),
           "k4_plan": plan, "consecutive_plan_rows": consecutive_rows([len(s) for s in seqs])}
    if other:
        o4 = ms["other_k4"]
        out.update({"other_k4_ms": o4, "other_k4_spread_ms": max(o4) - min(o4),
                    "other_k4_over_k4": min(o4) / min(k4), "k4_slower_than_other_by_ms": min(k4) - min(o4),
                    "other_hits_equal": same_hits(hits["k1"], hits["other_k4"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--qlen", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[64, 256, 1000, 4000])
    ap.add_argument("--mixed", type=int, default=256, help="queries of the mixed-length batch (0: skip it)")
    ap.add_argument("--c5mix", type=int, nargs="*", default=[1000, 2000],
                    help="query counts of bench.py's C5 mix (make_queries(0, n, 0)), multi-hit")
    ap.add_argument("--other-lib", default=None, help="libdcp_hip.so of another build: its kernel 4 runs alongside")
    a = ap.parse_args()
    dcp = _load_product()
    sizes = bench.core_sizes_for("c2", a.nprof)
    cfg = dcp.ProteinCfg(dcp.ENTRY_DIST_OCCUPANCY, 0.01)
    profs = [dcp.ProteinProfile.sample(0xC2 + p, int(sizes[p]), cfg, precision=64) for p in range(a.nprof)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    other = None
    if a.other_lib:
        other = dcp.Scanner(0, lib=load_other(dcp, a.other_lib))
        other.upload_db(profs)
    out = {"nprof": a.nprof, "qlen": a.qlen, "reps": a.reps, "other_lib": bool(other), "cases": []}
    pool = list(bench.make_queries(0, max(a.nq), a.qlen)) if a.nq else []
    for nq in a.nq:
        for multi in (True, False):
            out["cases"].append(run_case(dcp, sc, other, pool[:nq], multi, a.reps))
    if a.mixed:
        rng = np.random.default_rng(10_000)
        lens = np.exp(rng.uniform(np.log(100), np.log(10_000), a.mixed)).astype(int)
        lens[0], lens[-1] = 100, 10_000
        mixed = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]
        case = run_case(dcp, sc, other, mixed, True, a.reps)
        case["mixed_lengths"] = [int(lens.min()), int(lens.max())]
        out["cases"].append(case)
    for nq in a.c5mix:
        mix = bench.make_queries(0, nq, 0)
        case = run_case(dcp, sc, other, mix, True, a.reps, k1_reps=1)  # kernel 1 takes seconds here: one timed scan
        case["c5_mix"] = True
        case["plan_row_ratio"] = case["consecutive_plan_rows"] / case["k4_plan"]["sum_block_rows"]
        out["cases"].append(case)
    sc.close()
    if other:
        other.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
