"""What windows cost and what they buy (profiles/seq_windows/probe.txt).  Three legs, one per run:

  cut     upload(n) + cut_windows against upload of the same windows cut on the host (numpy slices, timed apart), at
          about 4 Mi bases of windows (64 sequences of 32 kbp, window 4 096, step 2 048), alternating in one process,
          one warm-up and three timed runs each; and the two kernels' own time from HIP events (dcp_launch_windows
          on buffers of the same shape, one warm-up and three launches).
  contig  one sequence of 128 kbp with planted genes against Pfam-like profiles (the C3 core sizes): scan ms,
          trace_paths ms and the growth of the device's memory in use across trace_paths (the traceback's work
          area, kept between calls) -- whole, and cut at 4 096 / 2 048.  Each case in a fresh context.
  mix     1 000 queries of the C5 length mix against the C5 profiles: Gcell/s of the query-lane scan whole and cut
          at 2 048 / 1 024 (float DB, kernel 3), and the batch plan of the double DB's query-lane kernel
          (last_scan_query_plan, kernel 4, fewer profiles) for both.

    python profiles/seq_windows_probe.py cut|contig|mix [--nprof N]
"""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

med = lambda xs: sorted(xs)[len(xs) // 2]


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


def hand_cut(dcp, seqs, window, step):
    return [s[o:o + window] for s in seqs for o in dcp.window_starts(len(s), window, step)]


def sample_profiles(dcp, sizes, precision=32):
    cfg = dcp.ProteinCfg(dcp.ENTRY_DIST_OCCUPANCY, 0.01)
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda p: dcp.ProteinProfile.sample(0xDEC1F0 + p, int(sizes[p]), cfg, f"PF{p:05d}",
                                                               precision=precision), range(len(sizes))))


class Hip:
    """The few HIP runtime calls the probe needs beside the library's own (the runtime the library is linked with)."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def check(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.check(self.lib.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 4))))
        self.check(self.lib.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1))  # hipMemcpyHostToDevice
        return p.value

    def free(self, p):
        self.check(self.lib.hipFree(C.c_void_p(p)))

    def event(self):
        e = C.c_void_p()
        self.check(self.lib.hipEventCreate(C.byref(e)))
        return e

    def record(self, e, stream):
        self.check(self.lib.hipEventRecord(e, C.c_void_p(stream)))

    def elapsed_ms(self, e0, e1):
        self.check(self.lib.hipEventSynchronize(e1))
        ms = C.c_float(0)
        self.check(self.lib.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value

    def free_bytes(self):
        free, total = C.c_size_t(0), C.c_size_t(0)
        self.check(self.lib.hipDeviceSynchronize())
        self.check(self.lib.hipMemGetInfo(C.byref(free), C.byref(total)))
        return free.value


class WindowArgs(C.Structure):  # struct dcp_window_args (csrc/dcp_seqs.h)
    _fields_ = [(n, C.c_void_p) for n in ("src_words", "src_woff", "src_len", "wfirst", "nwfirst", "words", "woff", "len",
                                          "wsrc", "wofs")] + \
               [("nsrc", C.c_uint), ("nwin", C.c_uint), ("nwords", C.c_uint32), ("window", C.c_uint32), ("step", C.c_uint32)]


def leg_cut(dcp, args):
    window, step, n, L = 4096, 2048, 64, 32768
    rng = np.random.default_rng(14)
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(n)]
    cat, off = flat(seqs)
    t0 = time.perf_counter()
    cut = hand_cut(dcp, seqs, window, step)
    cat2, off2 = flat(cut)
    t_host_cut = time.perf_counter() - t0
    sc = dcp.Scanner(0)
    dev, host = [], []
    for it in range(4):  # the first of each is the warm-up
        t0 = time.perf_counter()
        sc.upload_seqs_flat(cat, off)
        t1 = time.perf_counter()
        sc.cut_windows(window, step)
        t2 = time.perf_counter()
        assert sc.nseqs == len(cut)
        sc.upload_seqs_flat(cat2, off2)
        t3 = time.perf_counter()
        if it:
            dev.append((t2 - t0, t1 - t0, t2 - t1))
            host.append(t3 - t2)
    # the kernels alone, on the context's stream: buffers of the same shape (their contents do not change the work)
    lib = dcp.lib
    lib.dcp_launch_windows.restype = C.c_int
    lib.dcp_launch_windows.argtypes = [C.POINTER(WindowArgs), C.c_void_p]
    hip = Hip()
    cnt = len(cut) // n
    src_nw, win_nw = L // 16 + 3, window // 16 + 3
    u32 = lambda a: hip.upload(np.ascontiguousarray(a, np.uint32))
    nwin, nwords = n * cnt, n * cnt * win_nw
    d_src = u32(np.zeros(n * src_nw))
    d_swoff, d_slen = u32(np.arange(n) * src_nw), u32(np.full(n, L))
    d_first = u32(np.concatenate([np.arange(n) * cnt, np.arange(n) * cnt * win_nw]))
    d_words, d_idx = u32(np.zeros(nwords)), u32(np.zeros(4 * nwin))
    a = WindowArgs(d_src, d_swoff, d_slen, d_first, d_first + 4 * n, d_words, d_idx, d_idx + 4 * nwin, d_idx + 8 * nwin,
                   d_idx + 12 * nwin, n, nwin, nwords, window, step)
    ms = []
    for it in range(4):
        e0, e1 = hip.event(), hip.event()
        hip.record(e0, sc.stream)
        rc = lib.dcp_launch_windows(C.byref(a), sc.stream)
        hip.record(e1, sc.stream)
        t = hip.elapsed_ms(e0, e1)
        assert rc == 0
        if it:
            ms.append(t)
    for p in (d_src, d_swoff, d_slen, d_first, d_words, d_idx):
        hip.free(p)
    print(f"cut: {n} sequences of {L} bases, window {window}, step {step}: {nwin} windows, {int(off2[-1])} bases, {nwords} words")
    print("  device  upload(n) + cut_windows       ms: " + "  ".join(f"{1e3 * t[0]:.2f}" for t in dev) +
          f"   median {1e3 * med([t[0] for t in dev]):.2f}  (upload {1e3 * med([t[1] for t in dev]):.2f}"
          f" + cut_windows {1e3 * med([t[2] for t in dev]):.2f})")
    print("  host    upload(W) of hand-cut windows ms: " + "  ".join(f"{1e3 * t:.2f}" for t in host) +
          f"   median {1e3 * med(host):.2f}   (+ {1e3 * t_host_cut:.2f} ms once for the numpy slices)")
    print("  kernels window index + words          ms (HIP events): " + "  ".join(f"{t:.4f}" for t in ms) +
          f"   median {med(ms):.4f}  = {2 * 4 * nwords / (1e6 * med(ms)):.1f} GB/s of words read + written")
    sc.close()


def leg_contig(dcp, args):
    hip = Hip()
    L, ngenes = 128 << 10, 40
    sizes = bench.core_sizes_for("c3", args.nprof or 2000)
    profs = sample_profiles(dcp, sizes)
    rng = np.random.default_rng(128)
    seq = rng.integers(0, 4, L, dtype=np.uint8)
    for g in range(ngenes):  # one gene every 3 200 bases, from the profile's most likely codons (as bench.plant_hits)
        prof = profs[(g * 2654435761) % len(profs)]
        codon = prof.match_dist[:, 4:].reshape(-1, 5, 5, 5)[:, :4, :4, :4].reshape(-1, 64).argmax(axis=1)
        core = np.stack([(codon >> 4) & 3, (codon >> 2) & 3, codon & 3], axis=1).reshape(-1).astype(np.uint8)[:1800]
        seq[1000 + 3200 * g:1000 + 3200 * g + len(core)] = core
    print(f"contig: one sequence of {L} bases, {ngenes} planted genes, {len(profs)} profiles (C3 core sizes, sum {int(sizes.sum())})")
    for window, step in ((0, 0), (4096, 2048)):
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs([seq])
        if window:
            sc.cut_windows(window, step)
        scan_ms = []
        for it in range(3):
            sc.scan(True, False, 10.0, keep_scores=False)
            scan_ms.append(sc.last_scan_ms)
        hits = sc.hits()
        free0 = hip.free_bytes()
        t0 = time.perf_counter()
        paths, _ = sc.trace_paths(hits, True, False)
        t_trace = time.perf_counter() - t0
        grown = free0 - hip.free_bytes()
        t0 = time.perf_counter()
        sc.trace_paths(hits, True, False)
        t_again = time.perf_counter() - t0
        what = f"cut {window} / {step}: {sc.nseqs} windows" if window else "whole"
        print(f"  {what}: scan ms {'  '.join(f'{t:.2f}' for t in scan_ms)} (kernel {sc.last_scan_kernel}); {len(hits)} hits,"
              f" {sum(len(p) for p in paths)} steps; trace_paths {1e3 * t_trace:.1f} ms (again {1e3 * t_again:.1f} ms);"
              f" device memory grown by the traceback {grown / 2 ** 20:.0f} MiB")
        sc.close()


def leg_mix(dcp, args):
    nq = 1000
    seqs = bench.make_queries(0, nq, 0)
    for precision, nprof, kernel in ((32, args.nprof or 20000, dcp.KERNEL_QLANE2), (64, 300, dcp.KERNEL_QLANE64)):
        sizes = bench.core_sizes_for("c5", nprof)
        profs = sample_profiles(dcp, sizes, precision)
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        print(f"mix: {nq} queries of the C5 length mix ({sum(len(s) for s in seqs)} bases), {nprof} C5 profiles"
              f" (sum {int(sizes.sum())}), precision {precision}, kernel {kernel}")
        for window, step in ((0, 0), (2048, 1024)):
            sc.upload_seqs(seqs)
            if window:
                sc.cut_windows(window, step)
            ms = []
            for it in range(4):
                sc.scan(True, False, 10.0, keep_scores=False, kernel=kernel)
                if it:
                    ms.append(sc.last_scan_ms)
            assert sc.last_scan_kernel == kernel
            what = f"cut {window} / {step}: {sc.nseqs} windows" if window else "whole"
            plan = f"; plan {sc.last_scan_query_plan}" if kernel == dcp.KERNEL_QLANE64 else ""
            print(f"  {what}: {sc.cells} cells, scan ms {'  '.join(f'{t:.2f}' for t in ms)}, median {med(ms):.2f}"
                  f" = {sc.cells / (1e6 * med(ms)):.0f} Gcell/s; redo pairs {sc.last_scan_redo_pairs}{plan}")
        sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["cut", "contig", "mix"])
    ap.add_argument("--nprof", type=int, default=0)
    args = ap.parse_args()
    dcp = bench.load_product()
    {"cut": leg_cut, "contig": leg_contig, "mix": leg_mix}[args.leg](dcp, args)


if __name__ == "__main__":
    main()
