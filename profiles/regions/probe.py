"""What rescoring joined domains costs (profiles/regions/probe.txt).  Measured, not gated.

World (b) of DESIGN.md 14 as DESIGN.md 15 probes it (profiles/path_domains_probe.py): one sequence of 128 kbp with 40
planted genes against profiles of the C3 core sizes, cut at 4 096 / 2 048, multi-hit, threshold 10.  The windows' hits
are traced, split into domains and located; domain_regions (max_gap 0, flank 30) turns the domains into regions.  Then,
one warm-up and three timed runs each, medians:

  cut_regions   the call by the host clock (the source uploaded again before each run, not counted), and
                region_words_kernel alone between two HIP events (dcp_launch_regions on buffers of the same shape);
  scan_pairs    (region i, its profile) for every region: the synchronised call by the host clock and the kernels
                between the context's events (last_scan_ms);
  beside them, what gives the same scores without the two calls: a full scan() of the region batch against the whole
  DB, and trace_paths of the same pairs (whose alt scores are the pairs' scores).

    python profiles/regions/probe.py [--nprof N] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from path_domains_probe import contig, timed  # noqa: E402
from seq_windows_probe import Hip, med, sample_profiles  # noqa: E402


class RegionArgs(C.Structure):  # struct dcp_region_args (csrc/dcp_seqs.h)
    _fields_ = [(n, C.c_void_p) for n in ("src_words", "src_woff", "words", "woff", "len", "rsrc", "rbegin", "rminus")] + \
               [("n", C.c_uint), ("nwords", C.c_uint32)]


def kernel_ms(dcp, sc, src_len, reg):
    """region_words_kernel on buffers of the regions' shape (the words' contents do not change the work)"""
    lib = dcp.lib
    lib.dcp_launch_regions.restype = C.c_int
    lib.dcp_launch_regions.argtypes = [C.POINTER(RegionArgs), C.c_void_p]
    hip = Hip()
    u32 = lambda a: hip.upload(np.ascontiguousarray(a, np.uint32))
    nw = reg["len"].astype(np.int64) // 16 + 3
    woff = np.concatenate([[0], np.cumsum(nw)[:-1]])
    nwords = int(nw.sum())
    bufs = [u32(np.zeros(src_len // 16 + 3)), u32([0]), u32(np.zeros(nwords)), u32(woff), u32(reg["len"]), u32(reg["src"]),
            u32(reg["begin"]), u32(reg["minus"])]
    a = RegionArgs(*bufs, len(reg), nwords)
    ms = []
    for it in range(4):
        e0, e1 = hip.event(), hip.event()
        hip.record(e0, sc.stream)
        rc = lib.dcp_launch_regions(C.byref(a), sc.stream)
        hip.record(e1, sc.stream)
        t = hip.elapsed_ms(e0, e1)
        assert rc == 0
        if it:
            ms.append(t)
    for p in bufs:
        hip.free(p)
    return ms, nwords


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    window, step, flank = 4096, 2048, 30
    sizes = bench.core_sizes_for("c3", args.nprof)
    profs = sample_profiles(dcp, sizes)
    seq = contig(profs)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs([seq])
    sc.cut_windows(window, step)
    sc.scan(True, False, 10.0, keep_scores=False)
    hits = sc.hits()
    paths, _ = sc.trace_paths(hits, True, False)
    dom, _, _, _, _ = sc.path_domains(hits, paths, True, False)
    src, begin, end, minus = sc.locate_domains(hits, dom)
    profile = hits["profile_idx"][dom["path"]]
    (reg_of, reg), t_rule = timed(lambda: dcp.domain_regions(src, minus, profile, begin, end, [len(seq)], 0, flank))
    fmt = lambda ts: "  ".join(f"{t:.2f}" for t in ts) + f"   median {med(ts):.2f}"
    say(f"contig: one sequence of {len(seq)} bases, 40 planted genes, {len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())}),"
        f" cut {window} / {step}: {sc.nseqs} windows, {len(hits)} hits, {len(dom)} domains")
    say(f"  domain_regions(max_gap 0, flank {flank}): {len(reg)} regions of {int(reg['len'].min())} .. {int(reg['len'].max())} bases"
        f" ({int(reg['len'].sum())} in all), up to {int(reg['nparts'].max())} domains in one;  ms: {fmt(t_rule)}")

    def cut():
        sc.upload_seqs([seq])
        t0 = time.perf_counter()
        sc.cut_regions(reg["src"], reg["begin"], reg["len"], reg["minus"])
        return 1e3 * (time.perf_counter() - t0)

    t_cut = [cut() for _ in range(4)][1:]
    k_ms, nwords = kernel_ms(dcp, sc, len(seq), reg)
    say(f"  cut_regions            ms: {fmt(t_cut)}   ({nwords} words)")
    say(f"  region_words_kernel    ms (HIP events): {'  '.join(f'{t:.4f}' for t in k_ms)}   median {med(k_ms):.4f}")
    pairs_q = np.arange(len(reg), dtype=np.uint32)
    scan_ms = []

    def pairs():
        sc.scan_pairs(pairs_q, reg["profile"], True, False, float("-inf"))
        scan_ms.append(sc.last_scan_ms)
        return sc.hits()

    got, t_pairs = timed(pairs)
    cells = sc.cells
    say(f"  scan_pairs of {len(reg)} pairs  ms: {fmt(t_pairs)}   kernels (events) median {med(scan_ms[1:]):.3f};"
        f" {cells / 1e9:.3f} Gcell, {len(got)} records, {sc.last_scan_launches} launches")
    full_ms = []

    def full():
        sc.scan(True, False, float("-inf"), keep_scores=False)
        full_ms.append(sc.last_scan_ms)
        return sc.cells

    full_cells, t_full = timed(full)
    say(f"  scan() of the {len(reg)} regions x {len(profs)} profiles  ms: {fmt(t_full)}   kernels (events) median {med(full_ms[1:]):.3f};"
        f" {full_cells / 1e9:.3f} Gcell, kernel {sc.last_scan_kernel}")
    (tp, alt), t_trace = timed(lambda: sc.trace_paths(got, True, False))
    assert np.array_equal(alt.view(np.uint32), got["alt_loglik"].view(np.uint32))
    say(f"  trace_paths of the same {len(got)} pairs  ms: {fmt(t_trace)}   ({sum(len(p) for p in tp)} steps)")
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
