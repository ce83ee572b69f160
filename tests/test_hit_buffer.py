"""The float hit buffer at its edges (runs on a real MI355X).

Four float kernels write hit records behind `if (h < a.hit_cap)`: viterbi_rowsweep_kernel (grid and pair mode),
viterbi_mp_kernel, viterbi_segment_kernel (the pairs it finishes itself) and ql_publish (the three query-lane kernels).
Each is reached on purpose, with a DB and a mode in which no other site writes in that scan (what the API tells is
asserted: last_scan_kernel, launch_infos' R / W / nprofiles, last_scan_redo_pairs), and scanned into a caller buffer of
cap + 4096 records filled with a sentinel, for cap = n, n - 1 and 1 (n = the oracle's count of finite-LRT pairs; the
threshold makes each of them a hit): the counter reads n every time; with cap = n the records are the oracle's
filter exactly; with cap < n dcp_gpu_fetch_hits returns DCP_ENOMEM with *nhits == n and what was written are wanted
records; the 4096 records behind cap hold the sentinel bit for bit (`<=` for `<` lands there); and after
set_hit_buffer(None, 0, None) the context's own buffer gives the list again.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # before the product's library: both bring a HIP runtime, and torch must see the device too

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_gpu_parity import prof_eps
from test_qlane_edges import oracle_for, pfam_profiles, rand_of, u32

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0x5EA7C0DE
EVERY = -1e30  # lrt threshold: every finite LRT passes


def wanted_records(dcp, on, oa, q0=0):
    with np.errstate(invalid="ignore"):
        lrt = np.float32(-2) * (on - oa)
    q, p = np.nonzero(np.isfinite(lrt))  # row-major: sorted by (seq_idx, profile_idx)
    want = np.zeros(len(q), dcp.HIT_DTYPE)
    want["seq_idx"], want["profile_idx"], want["null_loglik"], want["alt_loglik"] = q + q0, p, on[q, p], oa[q, p]
    return want


def same_records(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in ("seq_idx", "profile_idx")) and \
        np.array_equal(u32(a["null_loglik"]), u32(b["null_loglik"])) and np.array_equal(u32(a["alt_loglik"]), u32(b["alt_loglik"]))


def check_buffer(dcp, sc, rescan, want):
    n = len(want)
    assert 1000 < n < 20000
    keys = set(zip(want["seq_idx"].tolist(), want["profile_idx"].tolist(), u32(want["null_loglik"]).tolist(),
                   u32(want["alt_loglik"]).tolist()))
    sent = np.array(SENTINEL, np.uint32).view(np.int32).item()
    try:
        for cap in (n, n - 1, 1):
            buf = torch.full((cap + GUARD, 4), sent, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            sc.set_hit_buffer(buf.data_ptr(), cap, cnt.data_ptr())
            rescan()
            assert int(cnt.cpu()[0]) == n, (cap, int(cnt.cpu()[0]), n)
            raw = np.ascontiguousarray(buf.cpu().numpy()).view(np.uint32)
            assert (raw[cap:] == SENTINEL).all(), (cap, np.argwhere(raw[cap:] != SENTINEL)[:4])
            out = np.zeros(n + 8, dcp.HIT_DTYPE)
            nh = C.c_uint(0)
            rc = sc._lib.dcp_gpu_fetch_hits(sc._c, out.ctypes.data, len(out), C.byref(nh))
            assert nh.value == n
            got = raw[:cap].reshape(-1).view(dcp.HIT_DTYPE)
            if cap == n:
                assert rc == 0 and same_records(out[:n], want)
                assert same_records(np.sort(got, order=["seq_idx", "profile_idx"]), want)
            else:
                assert rc == dcp.RC_ENOMEM
                assert set(zip(got["seq_idx"].tolist(), got["profile_idx"].tolist(), u32(got["null_loglik"]).tolist(),
                               u32(got["alt_loglik"]).tolist())) <= keys
    finally:
        sc.set_hit_buffer(None, 0, None)
    rescan()
    assert same_records(sc.hits(), want)


SITES = ["rowsweep_grid", "mp", "pair_mode", "segment", "qlane_w3", "qlane", "qlane2"]


@pytest.mark.parametrize("site", SITES)
def test_float_hit_buffer_edges(dcp, oracle32, site):
    """One writer of hit records per case (module docstring):
    rowsweep_grid  profiles of 129 .. 512 nodes, KERNEL_ROWSWEEP: one-wavefront classes R >= 3 in grid mode
    mp             profiles of at most 64 nodes, KERNEL_ROWSWEEP: that class always runs viterbi_mp_kernel
    pair_mode      every profile flagged (positive MD / DD) behind KERNEL_QLANE: every pair leaves the query-lane kernel
                   through the redo lists and is published by the row sweep's pair mode (redo pairs == all pairs)
    segment        test-hooks build, segmented sweep forced, profiles of 513 .. 1100 nodes, uni-hit: no pair has
                   feedback, so viterbi_segment_kernel publishes every pair itself
    qlane_w3 / qlane / qlane2   uni-hit (no redo pairs): ql_publish from the three-wavefront kernel (64 queries), the
                   single-stage one (200 queries) and the two-stage one"""
    rng = np.random.default_rng(8600 + SITES.index(site))
    sc = dcp.Scanner(0, lib=dcp.load_testhooks()) if site == "segment" else dcp.Scanner(0)
    multi, kernel = False, dcp.KERNEL_ROWSWEEP
    if site == "rowsweep_grid":
        sizes, nq, multi = [129, 192, 193, 256, 257, 300, 384, 448, 449, 512], 300, True
    elif site == "mp":
        sizes, nq, multi = [1, 2, 3, 17, 63, 64] + rng.integers(1, 65, 34).tolist(), 100, True
    elif site == "pair_mode":
        sizes, nq, multi, kernel = [20, 33, 40, 57, 64, 65, 80, 99, 120, 128, 129, 200], 300, True, dcp.KERNEL_QLANE
    elif site == "segment":
        sizes, nq = [513, 600, 768, 900, 1100], 600
    elif site == "qlane_w3":
        sizes, nq, kernel = rng.integers(1, 200, 60).tolist(), 64, dcp.KERNEL_QLANE
    else:
        sizes, nq = rng.integers(1, 200, 16).tolist(), 200
        kernel = dcp.KERNEL_QLANE if site == "qlane" else dcp.KERNEL_QLANE2
    profiles, params = pfam_profiles(dcp, rng, sizes)
    if site == "pair_mode":  # not a probability model: the delete path gains score, E(j) needs the delete states
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
        for i, (null, match, trans) in enumerate(params):
            trans = trans.copy()
            trans[1:sizes[i], 2], trans[1:sizes[i], 6] = np.float32(0.7), np.float32(0.4)
            profiles[i] = dcp.ProteinProfile.from_params(null, match, trans, cfg)
            prof_eps[id(profiles[i])] = cfg.epsilon
    seqs = rand_of(rng, [1, 2, 3] + rng.integers(4, 81, nq - 3).tolist())
    try:
        sc.upload_db(profiles, expand_on_host=True)
        sc.upload_seqs(seqs)
        if site == "segment":
            sc.test_set_rowsweep_variant(20, 4 | (2 << 24))  # segmented sweep: always
        on, oa = oracle_for(dcp, oracle32, sc, profiles, seqs, (multi, False), True, None, None, {})
        want = wanted_records(dcp, on, oa)

        def rescan():
            sc.scan(multi, False, EVERY, keep_scores=False, kernel=kernel)
            assert sc.last_scan_kernel == kernel
            infos = sc.launch_infos()
            redo = sc.last_scan_redo_pairs
            if site == "rowsweep_grid":
                assert redo == 0 and all(li["W"] == 1 and li["R"] >= 3 for li in infos)
                assert sum(li["nprofiles"] for li in infos) == len(profiles)
            elif site == "mp":
                assert redo == 0 and [(li["R"], li["W"], li["nprofiles"]) for li in infos] == [(1, 1, len(profiles))]
            elif site == "pair_mode":
                assert infos[0]["W"] == 0 and redo == len(seqs) * len(profiles)
            elif site == "segment":
                assert redo == 0 and all(li["W"] >= 4 for li in infos)
            else:
                assert infos[0]["W"] == 0 and redo == 0

        check_buffer(dcp, sc, rescan, want)
    finally:
        if site == "segment":
            sc.test_set_rowsweep_variant(-1, 0)
        sc.close()


def test_float_hits_past_the_first_and_the_device_buffer(dcp, oracle32):
    """As test_f64_edges does for double: 240 profiles of 1 .. 64 nodes (48 parameter sets and 192 copies) x 70 000
    queries of 1 .. 40 nt, row sweep (viterbi_mp_kernel) and KERNEL_QLANE2 (sequence indices past 16 bits, 1 094 groups).
    Both kernels' dense scores agree in bits and equal the oracle's on a sample of queries x every profile; a ranged scan
    with between 2^20 (Scanner.hits()' first buffer) and 2^22 hits comes back whole and equals the dense scores'
    filter; the full batch's more than 2^22 hits give DCP_ENOMEM with the true count, never a truncated list."""
    rng = np.random.default_rng(8700)
    ndist, nprof, nq = 48, 240, 70_000
    base, _ = pfam_profiles(dcp, rng, [1, 2, 3, 63, 64] + rng.integers(1, 65, ndist - 5).tolist())
    src = np.concatenate([np.arange(ndist), rng.integers(0, ndist, nprof - ndist)])
    lens = rng.integers(1, 41, nq)
    lens[[0, 65535, 65536, 65537, nq - 1]] = (1, 40, 17, 16, 40)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    cat = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    sc = dcp.Scanner(0)
    try:
        sc.upload_db([base[i] for i in src], expand_on_host=True)
        sc.upload_seqs_flat(cat, off)
        kernels = (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE2)
        sc.scan(True, False, 10.0, kernel=kernels[0])
        gn, ga = sc.scores()
        sc.scan(True, False, 10.0, kernel=kernels[1])
        assert sc.last_scan_kernel == dcp.KERNEL_QLANE2
        qn, qa = sc.scores()
        assert np.array_equal(u32(gn), u32(qn)) and np.array_equal(u32(ga), u32(qa))
        del qn, qa
        qs = np.array(sorted(set(rng.choice(nq, 600, replace=False).tolist()) |
                             {0, 1, 2, 65535, 65536, 65537, nq - 3, nq - 2, nq - 1}))
        sample = [cat[off[q]:off[q + 1]] for q in qs]
        on, oa = oracle_for(dcp, oracle32, sc, [base[i] for i in src], sample, (True, False), True, None, src, {})
        assert np.array_equal(u32(gn[qs]), u32(on)) and np.array_equal(u32(ga[qs]), u32(oa))
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(np.float32(-2) * (gn - ga))
        r0, r1 = 20_000, 32_000
        wq, wp = np.nonzero(finite[r0:r1])
        assert (1 << 20) < len(wq) <= (1 << 22) and int(finite.sum()) > (1 << 22)
        for k in kernels:
            sc.scan(True, False, EVERY, keep_scores=False, q_range=(r0, r1), kernel=k)
            h = sc.hits()
            assert len(h) == len(wq), (k, len(h), len(wq))
            assert np.array_equal(h["seq_idx"], wq + r0) and np.array_equal(h["profile_idx"], wp)
            assert np.array_equal(u32(h["null_loglik"]), u32(gn[h["seq_idx"], h["profile_idx"]]))
            assert np.array_equal(u32(h["alt_loglik"]), u32(ga[h["seq_idx"], h["profile_idx"]]))
            del h
            sc.scan(True, False, EVERY, keep_scores=False, kernel=k)
            buf = np.zeros(16, dcp.HIT_DTYPE)
            n = C.c_uint(0)
            assert dcp.lib.dcp_gpu_fetch_hits(sc._c, buf.ctypes.data, len(buf), C.byref(n)) == dcp.RC_ENOMEM
            assert n.value == int(finite.sum())
            with pytest.raises(dcp.DcpError) as e:
                sc.hits()
            assert e.value.rc == dcp.RC_ENOMEM
    finally:
        sc.close()
