"""The double-precision scan at its segment, pass and launch edges: viterbi64_kernel<R> (dcp_f64.hip) and its host
driver scan64 (dcp_gpu.hip) against the oracle's f64 Viterbi, at the shapes where the kernel changes code path.

  * core sizes at the launch groups' edges (R = 1 / 2 / 4 nodes per lane at 64 / 128 / 256 nodes) and the column
    segments' (256 nodes), lengths at the sequence words' (16 bases), profiles uploaded in a shuffled order;
  * multi-hit queries through segmented profiles: k copies of a planted domain, back to back (the best path
    re-enters B through E -> B) and spaced (through J -> B), which make the segmented sweep's B(j) fixed point
    take more than one pass.  That premise -- the oracle's own best path enters B k times -- is a CPU test;
  * the two stride loops: more than 2^24 pairs in one launch group, and a long query that puts several
    segmented pairs on each wavefront's boundary column;
  * sequences up to 2^20 - 1 nt, ranged scans, the LRT threshold in double, the hit buffer's 2^20 / 2^22 limits.

Tolerance as DESIGN §11 claims it: 1e-12 * max(1, |ref|), and -inf exactly where the oracle has -inf."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import B_STATE, ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM, J_STATE
from test_f64_scan import assert_scores_match, cfg64, oracle_scores, random_params
from test_gpu_parity import pfam_like_params, planted_query

FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (multi_hits, hmmer3_compat)


def make_profiles(dcp, oracle64, params, entries, eps=0.01):
    profs = [dcp.ProteinProfile.from_params(*prm, cfg64(dcp, e, eps), precision=64) for prm, e in zip(params, entries)]
    return profs, [oracle64.new(*prm, e, eps) for prm, e in zip(params, entries)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def hit_pairs(h):
    return list(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist()))


def positive_delete_params(rng, M):
    """Not a probability model: MD and DD gain score, so a delete state beats every match state of its row and
    decides E(j) (test_gpu_parity.test_positive_delete_transitions_keep_d_in_e, in double)."""
    null, match, trans = pfam_like_params(rng, M)
    trans = trans.astype(np.float64)
    trans[1:M, 2] = 0.7  # MD
    trans[1:M, 6] = 0.4  # DD
    return null, match, trans


# ---- planted multi-copy queries (the B(j) fixed point) ----------------------------------------------------------

PLANT_M = (257, 300, 513, 1024)  # all segmented: more than 256 nodes
PLANT_K = (1, 2, 3, 4, 5)
_FAMILIES = {}


def planted_family(oracle64, M):
    """Pfam-like parameters of core size M (seeded by M), the oracle's f64 profile of them, and queries carrying
    k = 1 .. 5 copies of the profile's planted core between 30-nt random flanks: back to back (spaced=False) and
    with 20-200 nt random spacers (spaced=True).  Returns (params, oracle profile, [(k, spaced, seq), ...])."""
    if M not in _FAMILIES:
        rng = np.random.default_rng(1000 + M)
        params = pfam_like_params(rng, M)
        op = oracle64.new(*params, ENTRY_DIST_OCCUPANCY, 0.01)
        core = planted_query(rng, op, M, flank=0)
        seqs = []
        for k in PLANT_K:
            for spaced in (False, True):
                parts = [rng.integers(0, 4, 30, dtype=np.uint8)]
                for i in range(k):
                    if i and spaced:
                        parts.append(rng.integers(0, 4, int(rng.integers(20, 201)), dtype=np.uint8))
                    parts.append(core)
                parts.append(rng.integers(0, 4, 30, dtype=np.uint8))
                seqs.append((k, spaced, np.concatenate(parts)))
        _FAMILIES[M] = (params, op, seqs)
    return _FAMILIES[M]


@pytest.mark.parametrize("M", PLANT_M)
def test_planted_copies_reenter_b(oracle64, M):
    """CPU, the premise of the fixed-point tests: on the oracle's own f64 best path, a query of k >= 2 planted
    copies enters B at least k times -- all but the first through E -> B or J -> B, which the segmented sweep's
    first pass (B = N + NB) does not have -- and the spaced copies pass through J."""
    _, op, seqs = planted_family(oracle64, M)
    for k, spaced, seq in seqs:
        if k < 2:
            continue
        op.setup(len(seq), True, False)
        rc, ll, path = op.viterbi(1, bytes(seq))
        assert rc == 0 and np.isfinite(ll)
        states = [s for s, _ in path]
        assert states.count(B_STATE) >= k, (M, k, spaced, states.count(B_STATE))
        if spaced:
            assert J_STATE in states, (M, k)


# ---- GPU ---------------------------------------------------------------------------------------------------------

EDGE_M = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1025,
          2049]
EDGE_L = [1, 2, 3, 4, 5, 6, 15, 16, 17, 31, 32, 33, 100, 1000]


@pytest.mark.gpu
def test_size_and_length_edges_shuffled(dcp, oracle64):
    """Every launch group's and segment's edge, three delete-heavy segmented profiles and one with positive MD / DD
    (D decides E(j), across segments), uploaded in a shuffled order: the group sort and the scatter back to the
    caller's index.  Every pair under all four flag combinations."""
    rng = np.random.default_rng(2049)
    kinds = [(M, "plain") for M in EDGE_M] + [(M, "delete") for M in (300, 640, 1100)] + [(513, "posdel")]
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    params, entries = [], []
    for i, (M, kind) in enumerate(kinds):
        params.append(positive_delete_params(rng, M) if kind == "posdel" else
                      random_params(rng, M, delete_heavy=kind == "delete"))
        entries.append((ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2])
    profs, oprofs = make_profiles(dcp, oracle64, params, entries)
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in rng.permutation(EDGE_L)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    for mh, h3 in FLAGS:
        sc.scan(mh, h3, 10.0)
        gn, ga = sc.scores()
        on, oa = oracle_scores(oracle64, oprofs, seqs, mh, h3)
        assert_scores_match(gn, on)
        assert_scores_match(ga, oa)
    sc.close()


@pytest.mark.gpu
def test_multi_hit_copies_through_segmented_profiles(dcp, oracle64):
    """k = 1 .. 5 planted copies, back to back and spaced, against Pfam-like profiles of 257 .. 1024 nodes: the
    segmented sweep must iterate B(j) to its fixed point (test_planted_copies_reenter_b shows the best paths
    need it).  Multi-hit with and without hmmer3_compat, and uni-hit, where one pass is exact."""
    fams = [planted_family(oracle64, M) for M in PLANT_M]
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * len(fams))
    oprofs = [f[1] for f in fams]
    rng = np.random.default_rng(5)
    seqs = [s for f in fams for _, _, s in f[2]] + [rng.integers(0, 4, L, dtype=np.uint8) for L in (1, 77, 3000)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    for mh, h3 in ((True, False), (True, True), (False, False)):
        sc.scan(mh, h3, 10.0)
        gn, ga = sc.scores()
        on, oa = oracle_scores(oracle64, oprofs, seqs, mh, h3)
        assert_scores_match(gn, on)
        assert_scores_match(ga, oa)
        # the planted queries are hits of their own profile
        q = 0
        for p, f in enumerate(fams):
            for _ in f[2]:
                assert -2 * (gn[q, p] - ga[q, p]) > 10.0, (p, q)
                q += 1
    sc.close()


@pytest.mark.gpu
def test_over_2_24_pairs_in_one_group_and_the_hit_buffer(dcp, oracle64):
    """240 profiles of 1-64 nodes (48 parameter sets, five copies each, shuffled) x 70 000 queries of 1-40 nt:
    16.8 M pairs in launch group R = 1, more than the 2^24 wavefronts it launches, so the last 22 784 pairs are
    each a wavefront's second; sequence indices past 16 bits.  Then the hit buffer: a ranged scan with between
    2^20 and 2^22 hits comes back whole through Scanner.hits(), and the full batch's 16.8 M hits overflow the
    device's 2^22 records: DCP_ENOMEM with the true count, never a truncated list."""
    rng = np.random.default_rng(224)
    ndist, ncopy, nq = 48, 5, 70_000
    sizes = [1, 2, 3, 63, 64] + rng.integers(1, 65, ndist - 5).tolist()
    params = [random_params(rng, M) for M in sizes]
    base, obase = make_profiles(dcp, oracle64, params,
                                [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(ndist)])
    of = rng.permutation(np.arange(ndist * ncopy) % ndist)  # caller index -> parameter set
    nprof = len(of)
    lens = rng.integers(1, 41, nq)
    lens[[0, 65535, 65536, 65537, nq - 1]] = (1, 40, 17, 16, 40)
    off = np.zeros(nq + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    cat = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    assert nprof * nq > 1 << 24
    # scan64 launches min(pairs, 2^24) wavefronts for the group; pair = profile * nq + query (all one group, the
    # caller's order): the pairs past 2^24 are the last profile's queries from here on
    tail0 = (1 << 24) - (nprof - 1) * nq
    sc = dcp.Scanner(0)
    sc.upload_db([base[i] for i in of])
    sc.upload_seqs_flat(cat, off)
    sc.scan(True, False, 10.0)
    gn, ga = sc.scores()
    for d in range(ndist):  # copies of one parameter set: the same bits
        cols = np.nonzero(of == d)[0]
        assert same_bits(gn[:, cols], np.repeat(gn[:, cols[:1]], len(cols), 1)), d
        assert same_bits(ga[:, cols], np.repeat(ga[:, cols[:1]], len(cols), 1)), d
    qs = set(rng.choice(nq, 600, replace=False).tolist()) | {0, 1, 2, 65535, 65536, 65537, nq - 3, nq - 2, nq - 1}
    qs |= {tail0 - 1, tail0, tail0 + 1}
    qs = np.array(sorted(qs))
    assert (qs >= tail0).sum() > 100
    seqs = [cat[off[q]:off[q + 1]] for q in qs]
    on, oa = oracle_scores(oracle64, obase, seqs, True, False)
    assert_scores_match(gn[qs], on[:, of])
    assert_scores_match(ga[qs], oa[:, of])

    lrt = -2 * (gn - ga)
    finite = np.isfinite(lrt)
    # more than 2^20 hits (Scanner.hits()' first buffer), at most 2^22 (the device's)
    r0, r1 = 20_000, 32_000
    sc.scan(True, False, -1e300, keep_scores=False, q_range=(r0, r1))
    h = sc.hits()
    want = np.nonzero(finite[r0:r1])
    assert (1 << 20) < len(h) <= (1 << 22) and len(h) == len(want[0])
    assert np.array_equal(h["seq_idx"], want[0] + r0) and np.array_equal(h["profile_idx"], want[1])
    assert same_bits(h["null_loglik"], gn[h["seq_idx"], h["profile_idx"]])
    assert same_bits(h["alt_loglik"], ga[h["seq_idx"], h["profile_idx"]])
    del h
    # more than 2^22: the true count, and no list
    sc.scan(True, False, -1e300, keep_scores=False)
    buf = np.zeros(16, dcp.HIT64_DTYPE)
    n = C.c_uint(0)
    assert dcp.lib.dcp_gpu_fetch_hits64(sc._c, buf.ctypes.data, len(buf), C.byref(n)) == dcp.RC_ENOMEM
    assert n.value == int(finite.sum()) > (1 << 22)
    with pytest.raises(dcp.DcpError) as e:
        sc.hits()
    assert e.value.rc == dcp.RC_ENOMEM
    sc.close()


@pytest.mark.gpu
def test_segmented_pairs_share_a_wavefront_column(dcp, oracle64):
    """One 200 000-nt query among 300 short ones against three segmented profiles: the boundary columns' budget
    (2^27 doubles, 5 per row) gives 134 wavefronts for 903 pairs, so every wavefront scores several pairs of
    different lengths in turn through one column.  Planted multi-copy queries among the short ones make some of
    them take a second pass.  Every pair against the oracle, multi-hit."""
    rng = np.random.default_rng(134)
    fams = [planted_family(oracle64, M) for M in (257, 300)]
    params = [f[0] for f in fams] + [random_params(rng, 513)]
    entries = [ENTRY_DIST_OCCUPANCY, ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM]
    profs, oprofs = make_profiles(dcp, oracle64, params, entries)
    short = [s for f in fams for k, _, s in f[2] if k <= 3]
    short += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(1, 400, 300 - len(short))]
    seqs = [short[i] for i in rng.permutation(len(short))]
    seqs.insert(123, rng.integers(0, 4, 200_000, dtype=np.uint8))
    waves = (1 << 27) // (5 * (200_000 + 1))
    assert waves == 134 and len(profs) * len(seqs) > 6 * waves
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    gn, ga = sc.scores()
    on, oa = oracle_scores(oracle64, oprofs, seqs, True, False)
    assert_scores_match(gn, on)
    assert_scores_match(ga, oa)
    sc.close()


@pytest.mark.gpu
def test_long_sequences(dcp, oracle64):
    """Queries of 2^20 - 1, 100 000, 25 000, 4 095 and 77 nt against a 40-node and a segmented 300-node profile,
    multi-hit.  The longest carries three planted copies of the 300-node profile's core far apart, so its
    segmented sweep iterates B(j) over a column of a million rows."""
    rng = np.random.default_rng(20)
    params300, op300, fam = planted_family(oracle64, 300)
    core = fam[0][2][30:-30]  # k = 1, back to back: the bare core
    params40 = random_params(rng, 40)
    profs, _ = make_profiles(dcp, oracle64, [params40], [ENTRY_DIST_UNIFORM])
    profs += make_profiles(dcp, oracle64, [params300], [ENTRY_DIST_OCCUPANCY])[0]
    oprofs = [oracle64.new(*params40, ENTRY_DIST_UNIFORM, 0.01), op300]
    longest = rng.integers(0, 4, (1 << 20) - 1, dtype=np.uint8)
    for at in (1000, 500_000, (1 << 20) - 2000):
        longest[at:at + len(core)] = core
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in (77, 4095, 25_000, 100_000)]
    seqs.insert(2, longest)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    gn, ga = sc.scores()
    on, oa = oracle_scores(oracle64, oprofs, seqs, True, False)
    assert_scores_match(gn, on)
    assert_scores_match(ga, oa)
    assert -2 * (gn[2, 1] - ga[2, 1]) > 10.0  # the planted copies are found
    sc.close()


def mixed_batch(dcp, oracle64, seed=55):
    """Profiles of every launch group, a segmented planted one among them, and 60 queries whose longest (12 000 nt)
    is query 37: a ranged scan's lmax, and so the boundary columns' stride, depends on whether it is in range."""
    rng = np.random.default_rng(seed)
    fam = planted_family(oracle64, 257)
    sizes = [20, 64, 100, 200, 256, 600]
    params = [random_params(rng, M) for M in sizes] + [fam[0]]
    entries = [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(len(params))]
    profs, oprofs = make_profiles(dcp, oracle64, params, entries)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(1, 3000, 60)]
    seqs[37] = rng.integers(0, 4, 12_000, dtype=np.uint8)
    for q, (k, _, s) in zip((5, 40, 55), [f for f in fam[2] if f[0] in (2, 3)][:3]):
        seqs[q] = s
    return profs, oprofs, seqs


@pytest.mark.gpu
def test_ranged_scans_and_repeats_same_bits(dcp, oracle64):
    """The same batch scanned twice, and through q_range over ranges with and without the longest query: the
    range's scores are the full scan's exact bits, and its hits carry batch-global seq_idx values in the range."""
    profs, oprofs, seqs = mixed_batch(dcp, oracle64)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    gn, ga = sc.scores()
    on, oa = oracle_scores(oracle64, oprofs, seqs, True, False)
    assert_scores_match(gn, on)
    assert_scores_match(ga, oa)
    sc.scan(True, False, 10.0)
    n2, a2 = sc.scores()
    assert same_bits(n2, gn) and same_bits(a2, ga)
    finite = np.isfinite(-2 * (gn - ga))
    for r0, r1 in ((0, 37), (30, 45), (38, 60), (37, 38), (59, 60)):
        sc.scan(True, False, -1e300, q_range=(r0, r1))
        n, a = sc.scores()
        assert same_bits(n[r0:r1], gn[r0:r1]) and same_bits(a[r0:r1], ga[r0:r1]), (r0, r1)
        h = sc.hits()
        want = np.nonzero(finite[r0:r1])
        assert np.array_equal(h["seq_idx"], want[0] + r0) and np.array_equal(h["profile_idx"], want[1]), (r0, r1)
        assert same_bits(h["null_loglik"], gn[h["seq_idx"], h["profile_idx"]])
        assert same_bits(h["alt_loglik"], ga[h["seq_idx"], h["profile_idx"]])
    sc.close()


@pytest.mark.gpu
def test_lrt_threshold_in_double(dcp, oracle64):
    """The LRT filter compares in double: a threshold of exactly a pair's LRT x keeps it, nextafter(x, +inf) drops
    it, where that threshold rounded to float would not exceed x.  dcp_gpu_set_lrt_threshold64's NaN sentinel
    takes (double) prm.lrt_threshold; -inf keeps every finite LRT and +inf none (kept iff finite and >=)."""
    profs, _, seqs = mixed_batch(dcp, oracle64, seed=66)
    lib = dcp.lib
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    gn, ga = sc.scores()
    lrt = -2 * (gn - ga)  # the kernel's expression: the same bits
    fin = np.isfinite(lrt)

    def hits_now():
        return set(hit_pairs(sc.hits()))

    def want(thr):
        return {(int(q), int(p)) for q, p in zip(*np.nonzero(fin & (lrt >= thr)))}

    up = np.nextafter(lrt, np.inf)
    cand = np.argwhere(fin & (up.astype(np.float32) <= lrt))
    assert len(cand) > 0
    q, p = (int(v) for v in cand[len(cand) // 2])
    x = float(lrt[q, p])
    for thr, kept in ((x, True), (float(np.nextafter(x, np.inf)), False)):
        sc.scan(True, False, thr, keep_scores=False)
        got = hits_now()
        assert ((q, p) in got) == kept, (x, thr)
        assert got == want(thr)
    # the NaN sentinel: the scan's float threshold, widened (set after a double threshold that would drop the pair)
    t_lo = np.float32(x)
    if t_lo > x:
        t_lo = np.nextafter(t_lo, np.float32(-np.inf))
    t_hi = np.nextafter(t_lo, np.float32(np.inf))
    assert t_lo <= x < t_hi
    for t32, kept in ((t_lo, True), (t_hi, False)):
        assert lib.dcp_gpu_set_lrt_threshold64(sc._c, float(np.nextafter(x, np.inf))) == dcp.RC_OK
        assert lib.dcp_gpu_set_lrt_threshold64(sc._c, float("nan")) == dcp.RC_OK
        prm = dcp.ScanParams(1, 0, float(t32), 0, dcp.KERNEL_AUTO)
        assert lib.dcp_gpu_scan(sc._c, C.byref(prm)) == dcp.RC_OK
        got = hits_now()
        assert ((q, p) in got) == kept, (x, float(t32))
        assert got == want(float(t32))
    # infinite thresholds
    sc.scan(True, False, -np.inf, keep_scores=False)
    assert hits_now() == want(-np.inf) and len(want(-np.inf)) == int(fin.sum())
    sc.scan(True, False, np.inf, keep_scores=False)
    assert len(sc.hits()) == 0
    sc.close()


@pytest.mark.gpu
def test_explicit_xtrans_refused_on_a_double_db(dcp):
    """Explicit special transitions are float: a scan of a double DB after set_xtrans is DCP_EINVAL (the
    length-derived ones again after the sequences are uploaded anew)."""
    sc = dcp.Scanner(0)
    sc.upload_db([dcp.ProteinProfile.sample(3, 300, precision=64)])
    seqs = ["ACGTACGTACGTAAAGGG", "GATTACA"]
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    ref = sc.scores()
    sc.set_xtrans(np.tile(dcp.xtrans(7, True, False), (2, 1)))
    with pytest.raises(dcp.DcpError) as e:
        sc.scan(True, False, 10.0)
    assert e.value.rc == dcp.RC_EINVAL
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    n, a = sc.scores()
    assert same_bits(n, ref[0]) and same_bits(a, ref[1])
    sc.close()
