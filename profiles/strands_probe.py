"""What both strands cost before the scan (profiles/strands_probe.txt): for 4 Mi bases of the C5 length mix
(log-uniform 100 nt .. 10 kbp) and of 1 kbp queries,

  device   dcp_gpu_seqs_upload(n) + dcp_gpu_seqs_add_revcomp      -- the reverse strand written from the resident words
  host     dcp_gpu_seqs_upload(2n) of the hand-doubled batch      -- the only way to both strands without the call;
                                                                     its numpy reverse complements are timed apart

alternating in one process, one warm-up and three timed runs each (wall time of the C calls, which return after
their copies), and the two kernels' own time from HIP events on the context's stream (dcp_launch_revcomp on the same
words, one warm-up and three launches).  The doubled scan itself is the same kernels on identical inputs.

    python profiles/strands_probe.py [--bases 4194304]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


def batches(total):
    mix, have, q = [], 0, 0
    while have < total:
        s = bench.make_queries(q, q + 1, 0)[0]
        mix.append(s)
        have += len(s)
        q += 1
    rng = np.random.default_rng(1)
    return {"c5 mix": mix, "1 kbp": [rng.integers(0, 4, 1000, dtype=np.uint8) for _ in range(total // 1000)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=4 << 20)
    args = ap.parse_args()
    import torch

    dcp = bench.load_product()
    lib = dcp.lib
    lib.dcp_launch_revcomp.restype = C.c_int
    lib.dcp_launch_revcomp.argtypes = [C.c_void_p] * 4 + [C.c_uint, C.c_uint32, C.c_void_p]
    sc = dcp.Scanner(0)
    stream = torch.cuda.ExternalStream(sc.stream)
    for name, seqs in batches(args.bases).items():
        n = len(seqs)
        cat, off = flat(seqs)
        t0 = time.perf_counter()
        rev = [dcp.revcomp(s) for s in seqs]
        cat2, off2 = flat(seqs + rev)
        t_host_rc = time.perf_counter() - t0
        dev, host = [], []
        for it in range(4):  # the first of each is the warm-up
            t0 = time.perf_counter()
            sc.upload_seqs_flat(cat, off)
            t1 = time.perf_counter()
            sc.add_reverse_strand()
            t2 = time.perf_counter()
            sc.upload_seqs_flat(cat2, off2)
            t3 = time.perf_counter()
            if it:
                dev.append((t2 - t0, t1 - t0, t2 - t1))
                host.append(t3 - t2)
        assert sc.nseqs == 2 * n
        # the kernels alone: the forward words as the upload packs them, on the context's stream
        nw = np.array([len(s) // 16 + 3 for s in seqs], np.int64)
        woff = np.zeros(2 * n, np.uint32)
        woff[1:n] = np.cumsum(nw)[:-1]
        nwords = int(nw.sum())
        ln = np.zeros(2 * n, np.uint32)
        ln[:n] = np.diff(off.astype(np.int64))
        d_words = torch.zeros(2 * nwords, dtype=torch.int32, device="cuda")
        d_woff = torch.from_numpy(woff.view(np.int32)).cuda()
        d_len = torch.from_numpy(ln.view(np.int32)).cuda()
        torch.cuda.synchronize()
        ms = []
        for it in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = lib.dcp_launch_revcomp(d_words.data_ptr(), d_words.data_ptr() + 4 * nwords, d_woff.data_ptr(),
                                        d_len.data_ptr(), n, nwords, sc.stream)
            e1.record(stream)
            e1.synchronize()
            assert rc == 0
            if it:
                ms.append(e0.elapsed_time(e1))
        med = lambda xs: sorted(xs)[len(xs) // 2]
        print(f"{name}: {n} sequences, {int(off[-1])} bases, {nwords} words")
        print("  device  upload(n) + add_revcomp  ms: " + "  ".join(f"{1e3 * t[0]:.2f}" for t in dev) +
              f"   median {1e3 * med([t[0] for t in dev]):.2f}  (upload {1e3 * med([t[1] for t in dev]):.2f}"
              f" + add_revcomp {1e3 * med([t[2] for t in dev]):.2f})")
        print("  host    upload(2n) hand-doubled  ms: " + "  ".join(f"{1e3 * t:.2f}" for t in host) +
              f"   median {1e3 * med(host):.2f}   (+ {1e3 * t_host_rc:.2f} ms once for the numpy reverse complements)")
        print("  kernels revcomp words + index    ms (HIP events): " + "  ".join(f"{t:.4f}" for t in ms) +
              f"   median {med(ms):.4f}  = {2 * 4 * nwords / (1e6 * med(ms)):.1f} GB/s of words read + written")
    sc.close()


if __name__ == "__main__":
    main()
