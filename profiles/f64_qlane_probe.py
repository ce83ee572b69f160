"""The f64 query-lane kernel (kernel 4) beside the f64 row sweep (kernel 1) of the same build, alternating in one
process, on the C2-sized job of f64_rate_probe.py: 1 000 profiles (bench.py's c2 core sizes, 100..300 nodes) against
64, 256, 1 000 and 4 000 queries of 300 nt, multi-hit and uni-hit, plus one mixed-length batch (100 nt .. 10 kbp).
Each case: one warm-up scan of each kernel, then `--reps` rounds of (kernel 1, kernel 4), HIP events around a scan's
launches (the redo launches included).  Prints one JSON line: every time, the best times' Gcell/s, kernel 1's spread
(max - min of its repeated times: the noise floor), the redo-pair count, and whether the two kernels' hit records
are equal.  python profiles/f64_qlane_probe.py [--nprof 1000 --qlen 300 --reps 3 --mixed 256]"""
import argparse
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


def run_case(dcp, sc, seqs, multi, reps):
    sc.upload_seqs(seqs)
    kernels = (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE64)
    ms = {k: [] for k in kernels}
    hits = {}
    redo = 0
    for r in range(reps + 1):
        for k in kernels:
            sc.scan(multi, False, 10.0, keep_scores=False, kernel=k)
            assert sc.last_scan_kernel == k
            if r:
                ms[k].append(sc.last_scan_ms)
            else:
                hits[k] = sc.hits(cap=1 << 22)
                if k == dcp.KERNEL_QLANE64:
                    redo = sc.last_scan_redo_pairs
    cells = sc.cells
    k1, k4 = ms[kernels[0]], ms[kernels[1]]
    return {"nq": len(seqs), "multi_hits": bool(multi), "cells": int(cells), "k1_ms": k1, "k4_ms": k4,
            "k1_gcells": cells / (min(k1) * 1e-3) / 1e9, "k4_gcells": cells / (min(k4) * 1e-3) / 1e9,
            "k1_spread_ms": max(k1) - min(k1), "k4_faster_by_ms": min(k1) - min(k4),
            "redo_pairs": int(redo), "hits": int(len(hits[kernels[0]])),
            "hits_equal": same_hits(hits[kernels[0]], hits[kernels[1]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--qlen", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[64, 256, 1000, 4000])
    ap.add_argument("--mixed", type=int, default=256, help="queries of the mixed-length batch (0: skip it)")
    a = ap.parse_args()
    dcp = _load_product()
    sizes = bench.core_sizes_for("c2", a.nprof)
    cfg = dcp.ProteinCfg(dcp.ENTRY_DIST_OCCUPANCY, 0.01)
    profs = [dcp.ProteinProfile.sample(0xC2 + p, int(sizes[p]), cfg, precision=64) for p in range(a.nprof)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    out = {"nprof": a.nprof, "qlen": a.qlen, "reps": a.reps, "cases": []}
    pool = list(bench.make_queries(0, max(a.nq), a.qlen))
    for nq in a.nq:
        for multi in (True, False):
            out["cases"].append(run_case(dcp, sc, pool[:nq], multi, a.reps))
    if a.mixed:
        rng = np.random.default_rng(10_000)
        lens = np.exp(rng.uniform(np.log(100), np.log(10_000), a.mixed)).astype(int)
        lens[0], lens[-1] = 100, 10_000
        mixed = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]
        case = run_case(dcp, sc, mixed, True, a.reps)
        case["mixed_lengths"] = [int(lens.min()), int(lens.max())]
        out["cases"].append(case)
    sc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
