"""What splitting hit paths into domains costs (profiles/path_domains/probe.txt).  Measured, not gated.

World (b) of DESIGN.md 14 (profiles/seq_windows_probe.py, leg contig): one sequence of 128 kbp with 40 planted genes
against profiles of the C3 core sizes, cut at 4 096 / 2 048, multi-hit, threshold 10.  Of the same hits, by the host
clock around the synchronised calls, one warm-up and three timed runs each, medians: trace_paths, decode_paths and
path_domains; the domain kernel alone between HIP events on the context's stream (path_domains_kernel_ms); then
locate_domains and merge_domains, with the number of domains before and after the merge.

    python profiles/path_domains_probe.py [--nprof N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402


def contig(profs, L=128 << 10, ngenes=40):
    """the contig of seq_windows_probe.leg_contig: one gene every 3 200 bases, the profile's most likely codons"""
    rng = np.random.default_rng(128)
    seq = rng.integers(0, 4, L, dtype=np.uint8)
    for g in range(ngenes):
        prof = profs[(g * 2654435761) % len(profs)]
        codon = prof.match_dist[:, 4:].reshape(-1, 5, 5, 5)[:, :4, :4, :4].reshape(-1, 64).argmax(axis=1)
        core = np.stack([(codon >> 4) & 3, (codon >> 2) & 3, codon & 3], axis=1).reshape(-1).astype(np.uint8)[:1800]
        seq[1000 + 3200 * g:1000 + 3200 * g + len(core)] = core
    return seq


def timed(call, runs=3):
    out, ts = None, []
    for it in range(runs + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        out = call()
        if it:
            ts.append(1e3 * (time.perf_counter() - t0))
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_domains", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    window, step = 4096, 2048
    sizes = bench.core_sizes_for("c3", args.nprof)
    profs = sample_profiles(dcp, sizes)
    seq = contig(profs)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs([seq])
    sc.cut_windows(window, step)
    sc.scan(True, False, 10.0, keep_scores=False)
    hits = sc.hits()
    say(f"contig: one sequence of {len(seq)} bases, 40 planted genes, {len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())}),"
        f" cut {window} / {step}: {sc.nseqs} windows, {len(hits)} hits")
    (paths, _), t_trace = timed(lambda: sc.trace_paths(hits, True, False))
    nsteps = sum(len(p) for p in paths)
    _, t_decode = timed(lambda: sc.decode_paths(hits, paths))
    kernel_ms = []

    def domains():
        out = sc.path_domains(hits, paths, True, False)
        kernel_ms.append(sc.path_domains_kernel_ms)
        return out

    (dom, dom_off, core, null, total), t_dom = timed(domains)
    assert np.array_equal(total.view(np.uint32), hits["alt_loglik"].view(np.uint32))
    fmt = lambda ts: "  ".join(f"{t:.2f}" for t in ts) + f"   median {med(ts):.2f}"
    say(f"  {nsteps} steps in {len(paths)} paths, {len(dom)} domains")
    say(f"  trace_paths   ms: {fmt(t_trace)}")
    say(f"  decode_paths  ms: {fmt(t_decode)}")
    say(f"  path_domains  ms: {fmt(t_dom)}")
    say(f"  domains_kernel ms (HIP events): {'  '.join(f'{t:.4f}' for t in kernel_ms[1:])}   median {med(kernel_ms[1:]):.4f}"
        f"  = {nsteps / (1e3 * med(kernel_ms[1:])):.1f} M steps/s")
    (src, begin, end, minus), t_loc = timed(lambda: sc.locate_domains(hits, dom))
    profile = hits["profile_idx"][dom["path"]]
    odds = core.astype(np.float64) - null.astype(np.float64)
    keep, t_merge = timed(lambda: dcp.merge_domains(src, minus, profile, begin, end, odds))
    say(f"  locate_domains ms: {fmt(t_loc)}")
    say(f"  merge_domains  ms: {fmt(t_merge)}")
    say(f"  domains before the merge {len(dom)}, after {int(keep.sum())}"
        f" (whole, uncut, the same contig gives 909 hits: profiles/seq_windows/probe.txt)")
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
