"""Cost of the double build's traceback (dcp_gpu_trace_paths64) beside the f64 scan of the same job.

Two jobs, multi-hit, double DB:
  c2     DESIGN §11's C2-sized job: 1 000 profiles (bench.py's c2 core sizes, 100..300 nodes) x 1 000 queries x 300 nt,
         one query in five carrying 90 nodes' best codons of a random profile (planted hits);
  mixed  200 profiles of the same sizes x 2 000 queries of 100 nt .. 10 kbp (log-uniform), half of them carrying one
         profile's full-length best codons: 1 000 planted hits, and the long queries' chance hits beside them.
Per job: one warm-up scan and trace, then the scan (HIP events: Scanner.last_scan_ms) and trace_paths of all its hits
(host clock around the call, which synchronises).  The forward pass and the walk are separate kernels
(viterbi64_kernel<R, true>, trace64_kernel): run under `rocprofv3 --kernel-trace --stats` for their split.
Prints one JSON line per job.   python profiles/trace64_probe.py [--jobs c2,mixed]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_product  # noqa: E402


def best_codons(prof, nodes):
    """per node the codon of the largest codon marginal of its match distribution (a 3-nt word scores f^4 of it)"""
    md = prof.parts64()[3]
    cod = md[:, 4:].reshape(-1, 5, 5, 5)[:, :4, :4, :4].reshape(-1, 64)
    best = np.argmax(cod[list(nodes)], axis=1)
    return np.stack([best >> 4, (best >> 2) & 3, best & 3], axis=1).astype(np.uint8).ravel()


def job(dcp, name, nprof, seqs_fn, rng):
    sizes = bench.core_sizes_for("c2", nprof)
    cfg = dcp.ProteinCfg(dcp.ENTRY_DIST_OCCUPANCY, 0.01)
    profs = [dcp.ProteinProfile.sample(0xC2 + p, int(sizes[p]), cfg, precision=64) for p in range(nprof)]
    seqs = seqs_fn(profs, rng)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    out = {"job": name, "nprof": nprof, "nq": len(seqs), "residues": int(sum(len(s) for s in seqs))}
    for rep in range(2):  # warm-up, then measured
        sc.scan(True, False, 10.0, keep_scores=False)
        hits = sc.hits()
        t0 = time.perf_counter()
        paths, _ = sc.trace_paths(hits)
        dt = time.perf_counter() - t0
    out.update(scan_s=sc.last_scan_ms * 1e-3, trace_s=dt,
               hits=int(len(hits)), steps=int(sum(len(p) for p in paths)),
               rows=int(sum(len(seqs[int(q)]) + 1 for q in hits["seq_idx"])),
               work_cells=int(sum((len(seqs[int(q)]) + 1) * profs[int(p)].core_size
                                  for q, p in zip(hits["seq_idx"], hits["profile_idx"]))))
    sc.close()
    return out


def c2_seqs(profs, rng):
    seqs = list(bench.make_queries(0, 1000, 300))
    for q in range(0, 1000, 5):
        p = int(rng.integers(len(profs)))
        dom = best_codons(profs[p], range(min(90, profs[p].core_size)))
        s = np.array(seqs[q], np.uint8).copy()
        s[15:15 + dom.size] = dom
        seqs[q] = s
    return seqs


def mixed_seqs(profs, rng):
    lens = np.exp(rng.uniform(np.log(100), np.log(10_000), 2000)).astype(int)
    seqs = []
    for q, L in enumerate(lens):
        s = rng.integers(0, 4, int(L), dtype=np.uint8)
        if q % 2 == 0:
            p = int(rng.integers(len(profs)))
            dom = best_codons(profs[p], range(profs[p].core_size))
            if dom.size + 10 > L:
                s = np.concatenate([s, rng.integers(0, 4, dom.size + 10 - int(L), dtype=np.uint8)])
            at = int(rng.integers(0, s.size - dom.size))
            s[at:at + dom.size] = dom
        seqs.append(s)
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="c2,mixed")
    a = ap.parse_args()
    dcp = _load_product()
    rng = np.random.default_rng(64)
    for name in a.jobs.split(","):
        if name == "c2":
            print(json.dumps(job(dcp, "c2", 1000, c2_seqs, rng)), flush=True)
        elif name == "mixed":
            print(json.dumps(job(dcp, "mixed", 200, mixed_seqs, rng)), flush=True)


if __name__ == "__main__":
    main()
