"""viterbi64_qlane_kernel (dcp_f64_qlane.hip, dcp_scan_params.kernel = 4 on a double DB) in bits.

Every comparison is made as uint64, with no tolerance, and twice: against viterbi64_kernel (kernel 1 on the same
context) over ALL pairs of the scan, and against the oracle's orc_dp_tables in double on the DB's own tables
(test_f64_bits.oracle_bits) over the pairs the CPU can afford.  Hit lists: every dcp_hit64 field bit-equal to
kernel 1's, and exactly the oracle's LRT filter with no margin.

  1. tile and table edges: core sizes 1 .. 2 KT + 1 and the launch groups' / segments' edges up to 4 096, uploaded
     shuffled, x lengths at the word and ring edges plus 1 000 and 10 007, all four flag combinations;
  2. batch shapes: 1 .. 1 000 queries, a mixed batch of 1 nt .. 12 kbp, a ranged scan that cuts a block of 256, the
     same scan twice and after a kernel-1 scan;
  3. the redo path: planted multi-copy queries in every launch group, with conditions on the test itself;
  4. redo-list overflow on the test-hooks build: the scan is repeated with the row sweep, last_scan_kernel == 1
     (what an overflowed kernel-2 scan of a float DB reports: finish_scan re-runs it with kernel 1);
  5. positive MD / DD and delete-heavy profiles;
  6. the threshold in double, NaN-LRT pairs, the hit buffer's 2^20 / 2^22 limits;
  7. the API's refusals, and tracebacks of kernel 4's hits."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import B_STATE, ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM
from test_f64_bits import Tables64, oracle_bits, u64
from test_f64_edges import EDGE_L, FLAGS, make_profiles, mixed_batch, planted_family, positive_delete_params
from test_f64_scan import random_params

pytestmark = pytest.mark.gpu

KT = 4  # DCP_F64_QL_KT


def scan_all(sc, kernel, mh, h3, thr=10.0, q_range=None):
    sc.scan(mh, h3, thr, q_range=q_range, kernel=kernel)
    gn, ga = sc.scores()
    return gn, ga, sc.hits()


def same_hits(a, b):
    return (len(a) == len(b) and np.array_equal(a["seq_idx"], b["seq_idx"]) and
            np.array_equal(a["profile_idx"], b["profile_idx"]) and
            np.array_equal(u64(a["null_loglik"]), u64(b["null_loglik"])) and
            np.array_equal(u64(a["alt_loglik"]), u64(b["alt_loglik"])))


def check4(dcp, oracle64, sc, tabs, seqs, opairs, mh, h3, thr=10.0, q_range=None):
    """Kernel 4, then kernel 1, on the same context: all pairs of the range and all hit fields in bits; then the
    oracle on the device's tables over `opairs`: bits, and the LRT filter exactly.  Returns (redo pairs, null, alt)."""
    gn, ga, h = scan_all(sc, dcp.KERNEL_QLANE64, mh, h3, thr, q_range)
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE64
    redo = sc.last_scan_redo_pairs
    assert sc.last_scan_ms > 0 and sc.last_scan_launches >= 1
    rn, ra, rh = scan_all(sc, dcp.KERNEL_ROWSWEEP, mh, h3, thr, q_range)
    assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP
    q0, q1 = q_range or (0, len(seqs))
    bad = np.argwhere((u64(gn[q0:q1]) != u64(rn[q0:q1])) | (u64(ga[q0:q1]) != u64(ra[q0:q1])))
    assert len(bad) == 0, (len(bad), [(int(q) + q0, int(p), gn[q + q0, p], rn[q + q0, p], ga[q + q0, p], ra[q + q0, p])
                                      for q, p in bad[:5]])
    assert same_hits(h, rh), (len(h), len(rh))
    opairs = [(q, p) for q, p in opairs if q0 <= q < q1]
    ref = oracle_bits(dcp, oracle64, tabs, seqs, opairs, mh, h3)
    got = set(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist()))
    for (q, p), (nl, al) in ref.items():
        assert u64(gn[q, p]) == u64(nl) and u64(ga[q, p]) == u64(al), (q, p, gn[q, p], nl, ga[q, p], al)
        with np.errstate(invalid="ignore"):
            lrt = -2 * (np.float64(nl) - np.float64(al))
        assert ((q, p) in got) == bool(np.isfinite(lrt) and lrt >= thr), (q, p, lrt, thr)
    return redo, gn, ga


def all_pairs(qs, ps):
    return [(q, p) for q in qs for p in ps]


def test_tile_and_table_edges(dcp, oracle64):
    """One-tile profiles, partial last tiles, core_size == ldk (no column behind the last tile: 64, 128, 256, 512,
    1 024, 4 096), every launch group of the double DB; lengths around the 16-base words and the five-row ring."""
    rng = np.random.default_rng(4104)
    sizes = list(range(1, 2 * KT + 2)) + [63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 2049, 4096]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    params = [random_params(rng, M) for M in sizes]
    entries = [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(len(sizes))]
    profs, _ = make_profiles(dcp, oracle64, params, entries)
    lens = [int(L) for L in rng.permutation(EDGE_L + [7, 9, 10, 11, 14, 10_007])]
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in lens]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    short = [q for q, L in enumerate(lens) if L <= 1000]
    qlong = lens.index(10_007)
    some = [p for p, M in enumerate(sizes) if M in (1, 5, 9, 64, 129, 513, 4096)]
    for i, (mh, h3) in enumerate(FLAGS):
        opairs = all_pairs(short, range(len(profs)))
        if i == 2:
            opairs += all_pairs([qlong], some)
        check4(dcp, oracle64, sc, tabs, seqs, opairs, mh, h3, thr=(10.0, 0.0)[i % 2])
    sc.close()


def test_batch_shapes(dcp, oracle64):
    """1 .. 1 000 queries (idle lanes in the last block, one and several blocks), then a ranged scan whose range
    cuts a block, the same scan twice, and again after a kernel-1 scan: the same bits."""
    rng = np.random.default_rng(256)
    sizes = [3, 37, 100, 260]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY] * 2)
    pool = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(1, 121, 1000)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    for nq in (1, 63, 64, 65, 255, 256, 257, 1000):
        seqs = pool[:nq]
        sc.upload_seqs(seqs)
        tabs = Tables64(sc, profs)
        qs = rng.choice(nq, min(nq, 40), replace=False).tolist()
        check4(dcp, oracle64, sc, tabs, seqs, all_pairs(qs, range(len(sizes))), True, False, thr=0.0)
    # nq = 1 000 is resident: a range that cuts the blocks of 256, twice, and around a kernel-1 scan
    gn, ga, h = scan_all(sc, dcp.KERNEL_QLANE64, True, False, 0.0)
    for r0, r1 in ((100, 700), (0, 257), (999, 1000)):
        _, n1, a1 = check4(dcp, oracle64, sc, tabs, pool, [], True, False, thr=0.0, q_range=(r0, r1))
        assert np.array_equal(u64(n1[r0:r1]), u64(gn[r0:r1])) and np.array_equal(u64(a1[r0:r1]), u64(ga[r0:r1]))
    n2, a2, h2 = scan_all(sc, dcp.KERNEL_QLANE64, True, False, 0.0)
    assert np.array_equal(u64(n2), u64(gn)) and np.array_equal(u64(a2), u64(ga)) and same_hits(h, h2)
    scan_all(sc, dcp.KERNEL_ROWSWEEP, True, False, 0.0)
    n3, a3, h3_ = scan_all(sc, dcp.KERNEL_QLANE64, True, False, 0.0)
    assert np.array_equal(u64(n3), u64(gn)) and np.array_equal(u64(a3), u64(ga)) and same_hits(h, h3_)
    sc.close()


def test_mixed_length_batch(dcp, oracle64):
    """Queries of 1 nt .. 12 kbp in one batch (blocks whose lanes end at very different rows), planted multi-copy
    queries among them, all four flag combinations; the oracle on the short queries and a sample of the long."""
    profs, _, seqs = mixed_batch(dcp, oracle64)
    rng = np.random.default_rng(12)
    seqs = list(seqs) + [rng.integers(0, 4, L, dtype=np.uint8) for L in (1, 2, 10_000)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    short = [q for q, s in enumerate(seqs) if len(s) <= 600]
    for mh, h3 in FLAGS:
        opairs = all_pairs(short, range(len(profs)))
        if mh and not h3:
            opairs += all_pairs([5, 37, 40, 55, len(seqs) - 1], range(len(profs)))
        check4(dcp, oracle64, sc, tabs, seqs, opairs, mh, h3)
    sc.close()


PLANT_ALL_GROUPS = (30, 100, 200, 257, 300)  # launch groups R = 1, 2, 4 and the segmented one


def test_redo_path(dcp, oracle64):
    """k = 1 .. 5 planted copies, back to back and spaced, of profiles of every launch group, among random queries.
    A pair whose oracle best path enters B more than once needs E -> B or J -> B, which the tiles' B0(j) does not
    have: it must come back through the redo list with the oracle's bits."""
    fams = [planted_family(oracle64, M) for M in PLANT_ALL_GROUPS]
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * len(fams))
    rng = np.random.default_rng(77)
    seqs, own = [], []
    for p, f in enumerate(fams):
        for _, _, s in f[2]:
            own.append((len(seqs), p))
            seqs.append(s)
    nplanted = len(seqs)
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(50, 600, 30)]
    order = rng.permutation(len(seqs))
    where = np.argsort(order)  # old index -> new
    seqs = [seqs[i] for i in order]
    own = [(int(where[q]), p) for q, p in own]
    # the premise, on the oracle's own best path (CPU)
    feedback = []
    for q, p in own:
        fams[p][1].setup(len(seqs[q]), True, False)
        rc, ll, path = fams[p][1].viterbi(1, bytes(seqs[q]))
        assert rc == 0 and np.isfinite(ll)
        if [s for s, _ in path].count(B_STATE) > 1:
            feedback.append((q, p))
    assert len(feedback) >= 4 * len(fams)  # k = 2 .. 5, at least one spacing each
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    opairs = sorted(set(own) | {(q, (p + 1) % len(fams)) for q, p in own} |
                    set(all_pairs([int(where[q]) for q in range(nplanted, len(seqs))], range(len(fams)))))
    npairs = len(seqs) * len(fams)
    for mh, h3 in ((True, False), (True, True)):
        redo, gn, ga = check4(dcp, oracle64, sc, tabs, seqs, opairs, mh, h3)
        assert 0 < redo < npairs, redo
        if not h3:
            assert redo >= len(feedback), (redo, len(feedback))
            for q, p in own:  # the planted queries are hits of their own profile
                assert -2 * (gn[q, p] - ga[q, p]) > 10.0
    redo, _, _ = check4(dcp, oracle64, sc, tabs, seqs, opairs, False, False)
    assert redo == 0
    sc.close()


def test_redo_list_overflow(dcp, oracle64):
    """The test-hooks build with lists of 3 pairs, fewer than the planted pairs: the kernel loses pairs, dcp_gpu_sync
    sees the overflow flag and repeats the scan with the row sweep -- exact bits and hit list, last_scan_kernel ==
    KERNEL_ROWSWEEP (as after an overflowed kernel-2 scan of a float DB).  With the lists restored, kernel 4 again."""
    fams = [planted_family(oracle64, M) for M in (100, 300)]
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * 2)
    seqs = [s for f in fams for _, _, s in f[2]]
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    rn, ra, rh = scan_all(sc, dcp.KERNEL_ROWSWEEP, True, False)
    gn, ga, h = scan_all(sc, dcp.KERNEL_QLANE64, True, False)
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE64
    full = sc.last_scan_redo_pairs
    assert full > 3
    sc.test_set_redo_cap(3)
    on, oa, oh = scan_all(sc, dcp.KERNEL_QLANE64, True, False)
    assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP
    for n, a, hh in ((gn, ga, h), (on, oa, oh)):
        assert np.array_equal(u64(n), u64(rn)) and np.array_equal(u64(a), u64(ra)) and same_hits(hh, rh)
    ref = oracle_bits(dcp, oracle64, tabs, seqs, all_pairs(range(len(seqs)), range(2)), True, False)
    for (q, p), (nl, al) in ref.items():
        assert u64(on[q, p]) == u64(nl) and u64(oa[q, p]) == u64(al), (q, p)
    sc.test_set_redo_cap(0)
    n2, a2, h2 = scan_all(sc, dcp.KERNEL_QLANE64, True, False)
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE64 and sc.last_scan_redo_pairs == full
    assert np.array_equal(u64(n2), u64(rn)) and np.array_equal(u64(a2), u64(ra)) and same_hits(h2, rh)
    sc.close()


def test_positive_delete_and_delete_heavy_profiles(dcp, oracle64):
    """MD / DD positive: a delete state decides E(j), also across tiles and in a partial last tile (the kernel takes
    E(j) over M and D of every node always); delete-heavy profiles, segmented for kernel 1 and not."""
    rng = np.random.default_rng(513)
    kinds = [(513, "posdel"), (7, "posdel"), (64, "posdel"), (300, "delete"), (640, "delete"), (1100, "delete"),
             (100, "delete")]
    params = [positive_delete_params(rng, M) if k == "posdel" else random_params(rng, M, delete_heavy=True)
              for M, k in kinds]
    profs, _ = make_profiles(dcp, oracle64, params, [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2]
                                                     for i in range(len(kinds))])
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in EDGE_L + [333]]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    for mh, h3 in ((True, False), (False, False), (True, True)):
        check4(dcp, oracle64, sc, tabs, seqs, all_pairs(range(len(seqs)), range(len(profs))), mh, h3)
    sc.close()


def test_threshold_in_double_and_nan_lrt(dcp, oracle64):
    """Kernel 4's epilogue filters in double: a threshold of exactly a pair's LRT keeps it, nextafter drops it, where
    that threshold rounded to float would not exceed it; the NaN sentinel takes (double) prm.lrt_threshold.  With
    epsilon = 0 a length that is no multiple of 3 has null = alt = -inf: a NaN LRT, never a hit at any threshold
    (queries of whole sense codons have a finite null score, so no NaN)."""
    profs, _, seqs = mixed_batch(dcp, oracle64, seed=66)
    lib = dcp.lib
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    K4 = dcp.KERNEL_QLANE64
    gn, ga, _ = scan_all(sc, K4, True, False)
    lrt = -2 * (gn - ga)
    fin = np.isfinite(lrt)

    def hits_now():
        h = sc.hits()
        return set(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist()))

    def want(thr):
        return {(int(q), int(p)) for q, p in zip(*np.nonzero(fin & (lrt >= thr)))}

    up = np.nextafter(lrt, np.inf)
    cand = np.argwhere(fin & (up.astype(np.float32) <= lrt))
    assert len(cand) > 0
    q, p = (int(v) for v in cand[len(cand) // 2])
    x = float(lrt[q, p])
    for thr, kept in ((x, True), (float(np.nextafter(x, np.inf)), False)):
        sc.scan(True, False, thr, keep_scores=False, kernel=K4)
        got = hits_now()
        assert ((q, p) in got) == kept, (x, thr)
        assert got == want(thr)
    t_lo = np.float32(x)
    if t_lo > x:
        t_lo = np.nextafter(t_lo, np.float32(-np.inf))
    t_hi = np.nextafter(t_lo, np.float32(np.inf))
    assert t_lo <= x < t_hi
    for t32, kept in ((t_lo, True), (t_hi, False)):
        assert lib.dcp_gpu_set_lrt_threshold64(sc._c, float(np.nextafter(x, np.inf))) == dcp.RC_OK
        assert lib.dcp_gpu_set_lrt_threshold64(sc._c, float("nan")) == dcp.RC_OK
        prm = dcp.ScanParams(1, 0, float(t32), 0, K4)
        assert lib.dcp_gpu_scan(sc._c, C.byref(prm)) == dcp.RC_OK
        got = hits_now()
        assert sc.last_scan_kernel == K4
        assert ((q, p) in got) == kept, (x, float(t32))
        assert got == want(float(t32))
    sc.scan(True, False, -np.inf, keep_scores=False, kernel=K4)
    assert hits_now() == want(-np.inf) and len(want(-np.inf)) == int(fin.sum())
    sc.scan(True, False, np.inf, keep_scores=False, kernel=K4)
    assert len(sc.hits()) == 0
    sc.close()

    rng = np.random.default_rng(30)
    sizes = [5, 64, 130, 300]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes], [ENTRY_DIST_OCCUPANCY] * 4, eps=0.0)
    lens = [4, 5, 6, 7, 99, 100, 300, 301, 1000]
    # sense codons (a stop codon makes every pair -inf at epsilon 0), then L % 3 more bases
    sense = np.array([c for c in range(64) if c not in (0b110000, 0b110010, 0b111000)])  # TAA, TAG, TGA
    seqs = []
    for L in lens:
        cod = rng.choice(sense, L // 3)
        s = np.stack([cod >> 4, (cod >> 2) & 3, cod & 3], 1).reshape(-1)
        seqs.append(np.concatenate([s, rng.integers(0, 4, L % 3)]).astype(np.uint8))
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    for thr in (-np.inf, -1e300, 0.0):
        _, gn, ga = check4(dcp, oracle64, sc, tabs, seqs, all_pairs(range(len(seqs)), range(4)), True, False, thr=thr)
        with np.errstate(invalid="ignore"):
            nan = np.isnan(-2 * (gn - ga))
        assert nan[[q for q, L in enumerate(lens) if L % 3]].all() and not nan[[q for q, L in enumerate(lens) if L % 3 == 0]].any()
        h = sc.hits()
        assert not nan[h["seq_idx"], h["profile_idx"]].any()
    sc.close()


def test_hit_buffer_limits(dcp, oracle64):
    """240 profiles of 1-64 nodes x 70 000 queries of 1-40 nt (test_f64_edges' shapes for kernel 1): all 16.8 M pairs
    in bits against kernel 1; a ranged scan with between 2^20 and 2^22 hits comes back whole; the full batch's hits
    overflow the device's 2^22 records: DCP_ENOMEM with the true count."""
    rng = np.random.default_rng(224)
    ndist, ncopy, nq = 48, 5, 70_000
    sizes = [1, 2, 3, 63, 64] + rng.integers(1, 65, ndist - 5).tolist()
    base, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                            [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(ndist)])
    of = rng.permutation(np.arange(ndist * ncopy) % ndist)
    lens = rng.integers(1, 41, nq)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    cat = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    sc = dcp.Scanner(0)
    sc.upload_db([base[i] for i in of])
    sc.upload_seqs_flat(cat, off)
    K4 = dcp.KERNEL_QLANE64
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    rn, ra = sc.scores()
    sc.scan(True, False, 10.0, kernel=K4)
    gn, ga = sc.scores()
    assert sc.last_scan_kernel == K4
    assert np.array_equal(u64(gn), u64(rn)) and np.array_equal(u64(ga), u64(ra))
    del rn, ra
    finite = np.isfinite(-2 * (gn - ga))
    r0, r1 = 20_000, 32_000
    sc.scan(True, False, -1e300, keep_scores=False, q_range=(r0, r1), kernel=K4)
    h = sc.hits()
    want = np.nonzero(finite[r0:r1])
    assert (1 << 20) < len(h) <= (1 << 22) and len(h) == len(want[0])
    assert np.array_equal(h["seq_idx"], want[0] + r0) and np.array_equal(h["profile_idx"], want[1])
    assert np.array_equal(u64(h["null_loglik"]), u64(gn[h["seq_idx"], h["profile_idx"]]))
    assert np.array_equal(u64(h["alt_loglik"]), u64(ga[h["seq_idx"], h["profile_idx"]]))
    del h
    sc.scan(True, False, -1e300, keep_scores=False, kernel=K4)
    buf = np.zeros(16, dcp.HIT64_DTYPE)
    n = C.c_uint(0)
    assert dcp.lib.dcp_gpu_fetch_hits64(sc._c, buf.ctypes.data, len(buf), C.byref(n)) == dcp.RC_ENOMEM
    assert n.value == int(finite.sum()) > (1 << 22)
    with pytest.raises(dcp.DcpError) as e:
        sc.hits()
    assert e.value.rc == dcp.RC_ENOMEM
    sc.close()


def test_api(dcp, oracle64):
    """Kernel 4 is the double DB's: DCP_EINVAL on a float DB; kernels 2 and 3 stay DCP_EINVAL on a double DB; explicit
    (float) special transitions then kernel 4 is DCP_EINVAL; a float fetch after a kernel-4 scan is DCP_EINVAL;
    dcp_gpu_trace_paths64 on kernel 4's hits gives the paths it gives on kernel 1's."""
    def einval(f):
        with pytest.raises(dcp.DcpError) as e:
            f()
        assert e.value.rc == dcp.RC_EINVAL

    seqs = ["ACGTACGTACGTAAAGGG", "GATTACA"]
    sc = dcp.Scanner(0)
    sc.upload_db([dcp.ProteinProfile.sample(3, 40)])
    sc.upload_seqs(seqs)
    einval(lambda: sc.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE64))
    sc.close()

    fam = planted_family(oracle64, 257)
    rng = np.random.default_rng(9)
    profs, _ = make_profiles(dcp, oracle64, [fam[0], random_params(rng, 40)], [ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM])
    qs = [s for _, _, s in fam[2][:6]] + [rng.integers(0, 4, 90, dtype=np.uint8)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(qs)
    for k in (dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2, 5):
        einval(lambda: sc.scan(True, False, 10.0, kernel=k))
    _, _, h4 = scan_all(sc, dcp.KERNEL_QLANE64, True, False, -1e300)
    assert sc.cells == sum(p.core_size for p in profs) * sum(len(s) for s in qs)
    f32 = np.zeros((len(qs), 2), np.float32)
    assert dcp.lib.dcp_gpu_fetch_scores(sc._c, f32.ctypes.data, f32.ctypes.data) == dcp.RC_EINVAL
    n = C.c_uint(0)
    buf = np.zeros(64, dcp.HIT_DTYPE)
    assert dcp.lib.dcp_gpu_fetch_hits(sc._c, buf.ctypes.data, len(buf), C.byref(n)) == dcp.RC_EINVAL
    paths4, alt4 = sc.trace_paths(h4)
    _, _, h1 = scan_all(sc, dcp.KERNEL_ROWSWEEP, True, False, -1e300)
    assert same_hits(h4, h1) and len(h4) > 0
    paths1, alt1 = sc.trace_paths(h1)
    assert np.array_equal(u64(alt4), u64(alt1)) and len(paths4) == len(paths1)
    for a, b in zip(paths4, paths1):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    sc.set_xtrans(np.tile(dcp.xtrans(7, True, False), (len(qs), 1)))
    einval(lambda: sc.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE64))
    sc.close()
