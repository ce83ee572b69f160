"""Double-precision tracebacks (dcp_gpu_trace_paths64) and product rows of the double build.

For every pair traced on the device, orc_dp_tables_path of the oracle's double build is fed the tables the double DB
holds (Tables64: the profile's f64 trans8, the match, insert and null tables read back from the device, dcp_xtrans64
of the pair) and its path must equal the device's step for step; the trace's score, the scan's and the oracle's must
be equal as uint64, and the path's fragment lengths must cover the query.  The CPU half pins the references: the
oracle's f64 walk on its own exported tables is orc_viterbi's path, and dcp_profile_decode of a double profile is the
oracle's double decode -- also where the float parts tie and the double ones do not.
"""
import numpy as np
import pytest

from oracle_py import B_STATE, ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM, NCODES
from test_f64_bits import Tables64, u64
from test_f64_edges import FLAGS, make_profiles, planted_family, positive_delete_params
from test_f64_scan import ALT_LL, NULL_LL, SEQ, cfg64, random_params
from test_products import CODONS
from test_trace_oracle import best_codons, gapped_params, gapped_query, identical_node_params, pfam_like_params
from test_trace_paths import free_device_bytes

gpu = pytest.mark.gpu
D_STATE_MSB = 2
EDGE_M = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 2049]


# ---- helpers ---------------------------------------------------------------------------------------------------

def trace_and_check(dcp, oracle64, sc, tabs, seqs, pairs, multi, h3, null_model=False, trace=None):
    """traces `pairs` [(q, p)] in that order; every path, score and length checked.  Returns the paths."""
    nl, al = sc.scores()
    hits = np.array([(q, p, nl[q, p], al[q, p]) for q, p in pairs], dcp.HIT64_DTYPE)
    paths, got = (trace or sc.trace_paths)(hits, multi, h3, null_model)
    assert got.dtype == np.float64 and len(paths) == len(pairs)
    xts = {}
    for (q, p), path, g in zip(pairs, paths, got):
        seq = bytes(seqs[q])
        if len(seq) not in xts:
            xts[len(seq)] = dcp.xtrans64(len(seq), multi, h3)
        t8, em, ei, en = tabs.t[p]
        onl, oal, apath, npath = oracle64.dp_tables_path(t8, em, ei, en, xts[len(seq)], seq)
        want_score, want = (onl, npath) if null_model else (oal, apath)
        scan = nl[q, p] if null_model else al[q, p]
        assert u64(g) == u64(scan) == u64(want_score), (q, p, g, scan, want_score)
        assert np.array_equal(path["state_id"], want[0]) and np.array_equal(path["seqlen"], want[1]), (
            q, p, len(path), len(want[0]))
        assert int(path["seqlen"].sum()) == len(seq)
    return paths


def finite_pairs(sc, nseqs, nprof, rng):
    _, al = sc.scores()
    pairs = [(q, p) for q in range(nseqs) for p in range(nprof) if np.isfinite(al[q, p])]
    return [pairs[i] for i in rng.permutation(len(pairs))]


def n_b(path):
    return int(np.sum(path["state_id"] == B_STATE))


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


# ---- GPU -------------------------------------------------------------------------------------------------------

@gpu
def test_group_and_segment_edges(dcp, oracle64, scanner):
    """every launch group's and segment's edge uploaded shuffled, queries of 1 .. 9 nt, 20 .. 400 nt, planted one- and
    two-domain hits and 3 000 nt: every pair with a finite score, hit or not, under all four flag combinations"""
    rng = np.random.default_rng(64)
    order = rng.permutation(len(EDGE_M))
    sizes = [EDGE_M[i] for i in order]
    params = [pfam_like_params(rng, M) for M in sizes]
    entries = [(ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM)[i % 2] for i in range(len(sizes))]
    profs, oprofs = make_profiles(dcp, oracle64, params, entries)
    flank = lambda n: rng.integers(0, 4, n, dtype=np.uint8).tobytes()
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in range(1, 10)]
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(20, 400, 4)]
    planted = []
    for M in (65, 257, 513):
        p = sizes.index(M)
        planted.append((len(seqs), p, 1))
        seqs.append(np.frombuffer(flank(20) + best_codons(oprofs[p], range(M)) + flank(9), np.uint8))
    p = sizes.index(129)
    d = best_codons(oprofs[p], range(129))
    planted.append((len(seqs), p, 2))
    seqs.append(np.frombuffer(flank(5) + d + flank(40) + d + flank(3), np.uint8))
    seqs.append(rng.integers(0, 4, 3000, dtype=np.uint8))
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    tabs = Tables64(scanner, profs)
    for multi, h3 in FLAGS:
        scanner.scan(multi, h3, 10.0)
        pairs = finite_pairs(scanner, len(seqs), len(profs), rng)
        assert len(pairs) > 150
        paths = trace_and_check(dcp, oracle64, scanner, tabs, seqs, pairs, multi, h3)
        for q, p, doms in planted:
            path = paths[pairs.index((q, p))]
            assert np.sum(path["state_id"] >> 14 == 0) >= sizes[p] // 2
            assert n_b(path) >= (doms if multi else 1)


@gpu
def test_planted_copies_take_several_passes(dcp, oracle64, scanner):
    """k = 1 .. 5 planted copies, back to back and spaced, through segmented profiles: the forward pass's B(j) fixed
    point takes several passes, and the work area must hold the last one's rows.  Each path enters B k times."""
    fams = [planted_family(oracle64, M) for M in (257, 513, 1024)]
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * len(fams))
    seqs, pairs, ks = [], [], []
    for p, f in enumerate(fams):
        for k, _, s in f[2]:
            pairs.append((len(seqs), p))
            ks.append(k)
            seqs.append(s)
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    tabs = Tables64(scanner, profs)
    for multi, h3 in ((True, False), (True, True)):
        scanner.scan(multi, h3, 10.0)
        paths = trace_and_check(dcp, oracle64, scanner, tabs, seqs, pairs, multi, h3)
        for path, k in zip(paths, ks):
            assert n_b(path) >= k


@gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
def test_ties(dcp, oracle64, scanner, multi, h3):
    """identical-node profiles with uniform entry against periodic queries (paths through different nodes score
    alike to the bit), delete-heavy profiles and the positive MD / DD one: the device takes the oracle's path"""
    rng = np.random.default_rng(23)
    ident = [1, 2, 40, 65, 129, 300]
    params = [identical_node_params(M, seed=M) for M in ident]
    params += [random_params(rng, M, delete_heavy=True) for M in (40, 300, 640)]
    params.append(positive_delete_params(rng, 513))
    entries = [ENTRY_DIST_UNIFORM] * len(ident) + [ENTRY_DIST_OCCUPANCY] * 4
    profs, oprofs = make_profiles(dcp, oracle64, params, entries)
    codon = best_codons(oprofs[0], [0])
    seqs = [np.frombuffer(s, np.uint8) for s in (codon, codon * 2, codon * 9, b"\x00\x01" * 11, b"\x02" * 9,
                                                 (codon + b"\x03") * 13, codon * 120)]
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (5, 150, 700)]
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    scanner.scan(multi, h3, 10.0)
    pairs = finite_pairs(scanner, len(seqs), len(profs), rng)
    paths = trace_and_check(dcp, oracle64, scanner, Tables64(scanner, profs), seqs, pairs, multi, h3)
    if not multi:  # one codon against identical nodes: E's first candidate (M_M) wins the tie
        for p, M in enumerate(ident):
            if (0, p) in pairs:
                st = paths[pairs.index((0, p))]["state_id"]
                assert list(st[-3:]) == [M, (3 << 14) | 4, (3 << 14) | 7]


@gpu
def test_null_model_paths(dcp, oracle64, scanner):
    rng = np.random.default_rng(31)
    profs, _ = make_profiles(dcp, oracle64, [pfam_like_params(rng, M) for M in (1, 64, 300)],
                             [ENTRY_DIST_OCCUPANCY] * 3)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 2, 3, 4, 5, 6, 9, 33, 400, 3001)]
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0)
    trace_and_check(dcp, oracle64, scanner, Tables64(scanner, profs), seqs,
                    [(q, p) for q in range(len(seqs)) for p in range(len(profs))], True, False, null_model=True)


@gpu
def test_paths_longer_than_the_estimate(dcp, oracle64, scanner):
    """3 and 8 planted copies across a 1 000-node profile's delete runs: longer than the 2L + 2M + 16 first
    capacity, traced once more at their exact counts"""
    rng = np.random.default_rng(1003)
    params = gapped_params(rng)
    profs, oprofs = make_profiles(dcp, oracle64, [params], [ENTRY_DIST_OCCUPANCY])
    seqs = [np.frombuffer(gapped_query(rng, oprofs[0], c), np.uint8) for c in (3, 8)]
    seqs.append(rng.integers(0, 4, 300, dtype=np.uint8))
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0)
    paths = trace_and_check(dcp, oracle64, scanner, Tables64(scanner, profs), seqs, [(0, 0), (2, 0), (1, 0)],
                            True, False)
    for path, q, copies in ((paths[0], 0, 3), (paths[2], 1, 8)):
        assert len(path) > 2 * len(seqs[q]) + 2 * 1000 + 16
        assert int(np.sum(path["state_id"] >> 14 == D_STATE_MSB)) == 980 * copies


@gpu
def test_rounds_order_and_duplicates(dcp, oracle64):
    """a budget so small that every hit takes its own round, then the default one: the same paths, in the caller's
    order, duplicates included"""
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    try:
        rng = np.random.default_rng(41)
        sizes = [1, 65, 129, 257, 513, 2049]
        profs, oprofs = make_profiles(dcp, oracle64, [pfam_like_params(rng, M) for M in sizes],
                                      [ENTRY_DIST_OCCUPANCY] * len(sizes))
        seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 7, 64, 333)]
        seqs.append(np.frombuffer(best_codons(oprofs[3], range(257)) * 2, np.uint8))
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        sc.scan(True, False, 10.0)
        pairs = finite_pairs(sc, len(seqs), len(profs), rng)
        pairs = pairs + pairs[:7] + [pairs[3]] * 3
        tabs = Tables64(sc, profs)
        got = []
        for budget in (1, 0):
            sc.test_set_trace_mode(0, budget)
            got.append(trace_and_check(dcp, oracle64, sc, tabs, seqs, pairs, True, False))
        assert all(np.array_equal(a, b) for a, b in zip(*got))
    finally:
        sc.test_set_trace_mode(0, 0)
        sc.close()


@gpu
def test_small_step_capacity_reports_the_needed_total(dcp, oracle64, scanner):
    rng = np.random.default_rng(51)
    profs, oprofs = make_profiles(dcp, oracle64, [pfam_like_params(rng, M) for M in (20, 300)],
                                  [ENTRY_DIST_OCCUPANCY] * 2)
    seqs = [rng.integers(0, 4, 90, dtype=np.uint8), np.frombuffer(best_codons(oprofs[1], range(300)), np.uint8)]
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0)
    nl, al = scanner.scores()
    hits = np.array([(q, p, nl[q, p], al[q, p]) for q in range(2) for p in range(2)], dcp.HIT64_DTYPE)
    paths, _ = scanner.trace_paths(hits)
    total = sum(len(p) for p in paths)
    call = scanner._lib.dcp_gpu_trace_paths64
    for cap in (0, 1, total - 1):
        off = np.zeros(len(hits) + 1, np.uint32)
        steps = np.zeros(max(cap, 1), dcp.STEP_DTYPE)
        rc = call(scanner._c, hits.ctypes.data, len(hits), 1, 0, 0, steps.ctypes.data, cap, off.ctypes.data, None)
        assert rc == dcp.RC_ENOMEM and off[-1] == total
        assert list(np.diff(off)) == [len(p) for p in paths]
    off = np.zeros(len(hits) + 1, np.uint32)
    steps = np.zeros(total, dcp.STEP_DTYPE)
    assert call(scanner._c, hits.ctypes.data, len(hits), 1, 0, 0, steps.ctypes.data, total, off.ctypes.data,
                None) == 0
    assert np.array_equal(steps, np.concatenate(paths))


@gpu
def test_hits_of_a_ranged_scan(dcp, oracle64, scanner):
    """the hit list of a ranged scan (absolute seq_idx) traced as it comes"""
    rng = np.random.default_rng(77)
    sizes = [40, 300]
    profs, oprofs = make_profiles(dcp, oracle64, [pfam_like_params(rng, M) for M in sizes],
                                  [ENTRY_DIST_OCCUPANCY] * 2)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(30, 300, 12)]
    for q in (5, 6, 9):
        p = q % 2
        seqs[q] = np.frombuffer(rng.integers(0, 4, 7, dtype=np.uint8).tobytes() +
                                best_codons(oprofs[p], range(sizes[p])), np.uint8)
    scanner.upload_db(profs)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0, q_range=(4, 11))
    h = scanner.hits()
    assert {(5, 1), (6, 0), (9, 1)} <= set(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist()))
    paths, got = scanner.trace_paths(h)
    t = Tables64(scanner, profs)
    for r, path, g in zip(h, paths, got):
        q, p = int(r["seq_idx"]), int(r["profile_idx"])
        assert 4 <= q < 11 and u64(g) == u64(r["alt_loglik"])
        t8, em, ei, en = t.t[p]
        _, oal, (st, ln), _ = oracle64.dp_tables_path(t8, em, ei, en, dcp.xtrans64(len(seqs[q]), True, False),
                                                      bytes(seqs[q]))
        assert u64(oal) == u64(g) and np.array_equal(path["state_id"], st) and np.array_equal(path["seqlen"], ln)


@gpu
def test_one_hit_whose_work_area_exceeds_2_31_doubles(dcp, oracle64, scanner):
    """M = 4096 against 180 kbp with two planted domains: 3 (L + 1) 4096 + 5 (L + 1) = 2.2e9 doubles (17.7 GB) of
    work area for one hit.  Its path must be a path of the device's tables whose score, summed step by step, is the
    scan's alt score in bits, and it must cover the query."""
    if free_device_bytes() < 24 << 30:
        pytest.skip("less than 24 GiB of free device memory")
    rng = np.random.default_rng(4096)
    profs, oprofs = make_profiles(dcp, oracle64, [pfam_like_params(rng, 4096)], [ENTRY_DIST_OCCUPANCY])
    L = 180_000
    assert 3 * (L + 1) * 4096 + 5 * (L + 1) > 1 << 31
    dom = np.frombuffer(best_codons(oprofs[0], range(4096)), np.uint8)
    seq = rng.integers(0, 4, L, dtype=np.uint8)
    seq[40_000:40_000 + dom.size] = dom
    seq[120_000:120_000 + dom.size] = dom
    scanner.upload_db(profs)
    scanner.upload_seqs([seq])
    scanner.scan(True, False, 10.0)
    nl, al = scanner.scores()
    (path,), got = scanner.trace_paths(np.array([(0, 0, nl[0, 0], al[0, 0])], dcp.HIT64_DTYPE))
    t8, em, ei, en = Tables64(scanner, profs).t[0]
    score = oracle64.path_score_tables(t8, em, ei, en, dcp.xtrans64(L, True, False), bytes(seq), path["state_id"],
                                       path["seqlen"])
    assert u64(got[0]) == u64(al[0, 0]) == u64(score)
    assert int(path["seqlen"].sum()) == L
    assert n_b(path) >= 2


@gpu
def test_errors(dcp, oracle64, scanner):
    """a float DB, the float call on a double DB, an index out of range, and a pair without a finite path"""
    rng = np.random.default_rng(3)
    scanner.upload_db([dcp.ProteinProfile.sample(1, 30)])
    scanner.upload_seqs([rng.integers(0, 4, 50, dtype=np.uint8)])
    scanner.scan(True, False, 10.0)
    off = np.zeros(3, np.uint32)
    steps = np.zeros(1000, dcp.STEP_DTYPE)
    h64 = np.array([(0, 0, 0.0, 0.0)], dcp.HIT64_DTYPE)
    assert scanner._lib.dcp_gpu_trace_paths64(scanner._c, h64.ctypes.data, 1, 1, 0, 0, steps.ctypes.data, 1000,
                                              off.ctypes.data, None) == dcp.RC_EINVAL
    # epsilon 0: every one-base word is -inf, so a 1-nt query has no finite alt path (20 GCA codons have one)
    profs, _ = make_profiles(dcp, oracle64, [pfam_like_params(rng, 30)], [ENTRY_DIST_OCCUPANCY], eps=0.0)
    scanner.upload_db(profs)
    scanner.upload_seqs([np.array([2], np.uint8), np.frombuffer(b"\x02\x01\x00" * 20, np.uint8)])
    scanner.scan(True, False, 10.0)
    h32 = np.array([(1, 0, 0.0, 0.0)], dcp.HIT_DTYPE)
    assert scanner._lib.dcp_gpu_trace_paths(scanner._c, h32.ctypes.data, 1, 1, 0, 0, steps.ctypes.data, 1000,
                                            off.ctypes.data, None) == dcp.RC_EINVAL
    for q, p in ((2, 0), (0, 1)):
        h = np.array([(1, 0, 0.0, 0.0), (q, p, 0.0, 0.0)], dcp.HIT64_DTYPE)
        assert scanner._lib.dcp_gpu_trace_paths64(scanner._c, h.ctypes.data, 2, 1, 0, 0, steps.ctypes.data, 1000,
                                                  off.ctypes.data, None) == dcp.RC_EINVAL
    _, al = scanner.scores()
    assert al[0, 0] == -np.inf and np.isfinite(al[1, 0])
    with pytest.raises(dcp.DcpError) as e:
        scanner.trace_paths(np.array([(1, 0, 0.0, al[1, 0]), (0, 0, 0.0, al[0, 0])], dcp.HIT64_DTYPE))
    assert e.value.rc == dcp.RC_EFAIL


@gpu
@pytest.mark.parametrize("entry", [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY])
def test_reference_golden(dcp, scanner, entry):
    """the reference's test sequence against sample(1, 2, 0.1) of the double build: 14 alt steps from S to T, the
    11-step null path from (R, 3) to (R, 2), the ten golden codons, and the alt score of the double build"""
    prof = dcp.ProteinProfile.sample(1, 2, cfg64(dcp, entry, 0.1), precision=64)
    scanner.upload_db([prof])
    scanner.upload_seqs([SEQ])
    scanner.scan(True, False, 10.0)
    nl, al = scanner.scores()
    hit = np.array([(0, 0, nl[0, 0], al[0, 0])], dcp.HIT64_DTYPE)
    (p,), alt = scanner.trace_paths(hit)
    (npath,), nul = scanner.trace_paths(hit, null_model=True)
    assert u64(nul[0]) == u64(nl[0, 0]) and abs(nul[0] - NULL_LL) < 1e-10
    assert len(npath) == 11
    assert [(int(s["state_id"]), int(s["seqlen"])) for s in (npath[0], npath[10])] == [(3 << 14, 3), (3 << 14, 2)]
    assert u64(alt[0]) == u64(al[0, 0]) and abs(alt[0] - ALT_LL[entry]) < 1e-10
    assert len(p) == 14
    assert (p[0]["state_id"], p[0]["seqlen"]) == ((3 << 14) | 1, 0)
    assert (p[13]["state_id"], p[13]["seqlen"]) == ((3 << 14) | 7, 0)
    row = prof.prod_row(SEQ, p)
    assert [m.split(",")[2] for m in row[:-1].split("\t")[8].split(";") if m.split(",")[0]] == CODONS


# ---- CPU -------------------------------------------------------------------------------------------------------

def all_words():
    out = []
    for n in range(1, 6):
        for v in range(4 ** n):
            out.append(bytes((v >> (2 * (n - 1 - i))) & 3 for i in range(n)))
    assert len(out) == NCODES
    return out


@pytest.mark.parametrize("entry", [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY])
def test_decode_in_double(dcp, oracle64, entry):
    """every one of the 1 364 words decoded by M, I and N / J / C states of sampled double profiles: the oracle's
    double decode's codon, or at an exact tie one whose joint probability is the best within 1e-12"""
    M = 7
    prof = dcp.ProteinProfile.sample(11 + entry, M, cfg64(dcp, entry, 0.01), precision=64)
    op = oracle64.sample(11 + entry, M, entry, 0.01)
    states = [1, 4, M, (1 << 14) | 2, (3 << 14) | 2, (3 << 14) | 5, (3 << 14) | 6]
    for sid in states:
        for w in all_words():
            lp, want = op.decode(w, sid)
            got = prof.decode(np.frombuffer(w, np.uint8), sid)
            if got != want:
                assert abs(op.codon_lprob(w, sid, got) - lp) <= 1e-12, (sid, w, got, want)


AA = "ACDEFGHIKLMNPQRSTVWY"


def float_tie_params(delta=1e-9):
    """one node whose alanine and glycine (four codons each; GCA and GGA the only ones with an A) are 0.45 likely,
    alanine ahead by `delta` in log: less than a float can hold at that value, far more than double rounding"""
    p = np.full(20, 0.1 / 18)
    p[AA.index("A")] = p[AA.index("G")] = 0.45
    lp = np.log(p)
    lp[AA.index("A")] += delta
    trans = np.log(np.array([[0.9, 0.05, 0.05, 0.5, 0.5, 0.5, 0.5]] * 2))
    trans[0, 6] = trans[1, 2] = trans[1, 6] = -np.inf
    return lp.copy(), lp[None, :].copy(), trans


def test_a_tie_only_in_float_decodes_as_the_double_build(dcp, oracle64):
    """the one-base fragment "A": GCA and GGA score their codon probability alone.  Rounded to float, those tie (and
    the float decode keeps the later codon, GGA); in double alanine's is larger, and the double build decodes GCA"""
    null, match, trans = float_tie_params()
    null = np.log(np.full(20, 1 / 20))
    prof = dcp.ProteinProfile.from_params(null, match, trans, cfg64(dcp, ENTRY_DIST_OCCUPANCY, 0.01), precision=64)
    _, nd, _, md = prof.parts64()
    gca, gga = 4 + 2 * 25 + 1 * 5 + 0, 4 + 2 * 25 + 2 * 5 + 0
    assert 1e-12 < md[0, gca] - md[0, gga] and np.float32(md[0, gca]) == np.float32(md[0, gga])
    op = oracle64.new(null, match, trans, ENTRY_DIST_OCCUPANCY, 0.01)
    assert op.decode(b"\x00", 1)[1] == prof.decode("A", 1) == "GCA"
    # the same tie in the null distribution: N, J and C states
    null2, _, _ = float_tie_params()
    prof2 = dcp.ProteinProfile.from_params(null2, match, trans, cfg64(dcp, ENTRY_DIST_OCCUPANCY, 0.01),
                                           precision=64)
    _, nd2, _, _ = prof2.parts64()
    assert 1e-12 < nd2[gca] - nd2[gga] and np.float32(nd2[gca]) == np.float32(nd2[gga])
    op2 = oracle64.new(null2, match, trans, ENTRY_DIST_OCCUPANCY, 0.01)
    for sid in ((3 << 14) | 2, (3 << 14) | 5, (3 << 14) | 6):
        assert op2.decode(b"\x00", sid)[1] == prof2.decode("A", sid) == "GCA"
    # and the product row writes it
    row = prof.prod_row("A", np.array([((3 << 14) | 1, 0, 0), (3 << 14 | 3, 0, 0), (1, 1, 0), ((3 << 14) | 4, 0, 0),
                                       ((3 << 14) | 7, 0, 0)], dcp.STEP_DTYPE))
    assert "A,M1,GCA,A" in row


def check_pair64(orc, prof, seq, setup=None):
    """the oracle's f64 walk on the profile's exported tables == orc_viterbi of the double build, paths and scores
    in bits; returns the alt path"""
    if setup is not None:
        assert prof.setup(len(seq), *setup) == 0
    t8, em, ei, en, xt = prof.export()
    rc, ll, want = prof.viterbi(1, seq)
    rc0, ll0, want0 = prof.viterbi(0, seq)
    assert rc == 0 and rc0 == 0
    nl, al, apath, npath = orc.dp_tables_path(t8, em, ei, en, xt, seq)
    assert u64(al) == u64(ll) and u64(nl) == u64(ll0), (al, ll, nl, ll0)
    assert list(zip(*[a.tolist() for a in apath])) == want
    assert list(zip(*[a.tolist() for a in npath])) == want0
    return want


@pytest.mark.parametrize("M", [2, 5, 64, 65, 257])
def test_oracle_walk_on_its_tables_is_the_f64_viterbi(oracle64, M):
    rng = np.random.default_rng(M)
    for entry in (ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY):
        prof = oracle64.sample(M + entry, M, entry, 0.01)
        for L in (1, 2, 5, 16, 100):
            seq = rng.integers(0, 4, L, dtype=np.uint8).tobytes()
            for multi, h3 in FLAGS:
                check_pair64(oracle64, prof, seq, (multi, h3))


def test_oracle_walk_on_planted_ties_and_long_paths(oracle64):
    rng = np.random.default_rng(8)
    prof = oracle64.new(*pfam_like_params(rng, 60))
    dom = best_codons(prof, range(60))
    for seq in (dom, dom * 3, rng.integers(0, 4, 9, dtype=np.uint8).tobytes() + dom + dom[:40]):
        for multi, h3 in FLAGS:
            assert check_pair64(oracle64, prof, seq, (multi, h3))
    null, match, trans = identical_node_params(40)
    prof = oracle64.new(null, match, trans, ENTRY_DIST_UNIFORM)
    codon = best_codons(prof, [0])
    for seq in (codon, codon * 7, (codon + b"\x03") * 9):
        for multi, h3 in FLAGS:
            check_pair64(oracle64, prof, seq, (multi, h3))
    prof = oracle64.new(*gapped_params(rng))
    path = check_pair64(oracle64, prof, gapped_query(rng, prof, 3), (True, False))
    assert sum(1 for s, _ in path if s >> 14 == D_STATE_MSB) == 980 * 3
