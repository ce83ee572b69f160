"""Both strands: dcp_seq_revcomp on the host, and revcomp_words_kernel (csrc/dcp_seqs.hip) behind
dcp_gpu_seqs_add_revcomp / Scanner.add_reverse_strand on the device.

CPU: the host map against a numpy restatement.
GPU, one DB per precision (about 30 sampled profiles, core sizes on the launch groups' edges) and queries whose lengths
sit on the word and double-word edges of the kernel's 64-bit shift:
  1. the words the kernel wrote, bit for bit, pad words and tail bits included;
  2. a batch doubled on the device scans to the bits of the same batch doubled by hand, on every kernel and flag set;
  3. a hit that exists on the minus strand only comes back with the original query's bits, path and product row;
  4. ranged scans (minus strand only, straddling n) and a 300-query mixed-length batch doubled through the
     query-lane kernels;
  5. the refusals of the contract."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_f64_scan import random_params
from test_gpu_parity import pfam_like_params, planted_query

FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (multi_hits, hmmer3_compat)
EDGE_M = (1, 2, 64, 65, 128, 129, 257, 512, 513)
EDGE_L = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 1000, 10007)
PRECISIONS = (32, 64)


def np_revcomp(ids):
    ids = np.asarray(ids, np.uint8)
    return (3 - ids[::-1]).astype(np.uint8)


def host_words(ids):
    """dcp_gpu_seqs_upload's packing: base i in bits 2 (i & 15) of word i >> 4, L // 16 + 3 words."""
    ids = np.asarray(ids, np.uint64)
    w = np.zeros(len(ids) // 16 + 3, np.uint64)
    i = np.arange(len(ids))
    np.bitwise_or.at(w, i >> 4, ids << ((i & 15) * 2).astype(np.uint64))
    return w.astype(np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- CPU ---------------------------------------------------------------------------------------------------------


def test_revcomp_equals_numpy(dcp):
    rng = np.random.default_rng(7)
    for L in (1, 2, 3, 15, 16, 17, 100, 10007):
        s = rng.integers(0, 4, L, dtype=np.uint8)
        assert np.array_equal(dcp.revcomp(s), np_revcomp(s))
        assert np.array_equal(dcp.revcomp(bytes(s)), np_revcomp(s))


def test_revcomp_is_an_involution(dcp):
    rng = np.random.default_rng(8)
    for L in (1, 16, 33, 999):
        s = rng.integers(0, 4, L, dtype=np.uint8)
        assert np.array_equal(dcp.revcomp(dcp.revcomp(s)), s)


def test_revcomp_of_all_a_is_all_t(dcp):
    assert np.array_equal(dcp.revcomp(np.zeros(37, np.uint8)), np.full(37, 3, np.uint8))


def test_acgt_is_its_own_revcomp(dcp):
    acgt = dcp.encode_seq("ACGT")
    assert np.array_equal(dcp.revcomp(acgt), acgt)
    assert len(dcp.revcomp(np.zeros(0, np.uint8))) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------

_WORLDS = {}


def world(dcp, precision):
    """(profiles, queries): 30 sampled profiles, the edge core sizes among them, and the edge-length queries, a
    reverse-complement palindrome and an all-A query."""
    if precision not in _WORLDS:
        rng = np.random.default_rng(950 + precision)
        sizes = list(EDGE_M) + [int(m) for m in rng.integers(3, 400, 30 - len(EDGE_M))]
        sizes = [sizes[i] for i in rng.permutation(len(sizes))]
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
        # (protein_profile_sample takes two nodes at least: the one-node profile is built from random parameters)
        profs = [dcp.ProteinProfile.sample(300 + i, M, cfg, f"P{i:02d}", precision=precision) if M > 1 else
                 dcp.ProteinProfile.from_params(*random_params(rng, 1), cfg, f"P{i:02d}", precision=precision)
                 for i, M in enumerate(sizes)]
        seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in EDGE_L]
        half = rng.integers(0, 4, 21, dtype=np.uint8)
        seqs.append(np.concatenate([half, np_revcomp(half)]))  # its own reverse complement
        seqs.append(np.zeros(40, np.uint8))
        _WORLDS[precision] = (profs, seqs)
    return _WORLDS[precision]


def kernels_of(dcp, precision):
    return (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE64) if precision == 64 else \
        (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2)


@pytest.mark.gpu
def test_words_of_the_reverse_strand(dcp):
    """fetch_seq and the raw words (test-hooks build) of every resident sequence after add_reverse_strand."""
    _, seqs = world(dcp, 32)
    n = len(seqs)
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    assert sc.strands == 0
    sc.upload_seqs(seqs)
    assert sc.strands == 1 and sc.nseqs == n
    sc.add_reverse_strand()
    assert sc.strands == 2 and sc.nseqs == 2 * n
    for q, s in enumerate(seqs):
        rc = np_revcomp(s)
        assert np.array_equal(sc.fetch_seq(q), s), q
        assert np.array_equal(sc.fetch_seq(n + q), rc), q
        assert np.array_equal(sc.fetch_seq(n + q), dcp.revcomp(s)), q
        assert np.array_equal(sc.test_seq_words(q), host_words(s)), q
        got, want = sc.test_seq_words(n + q), host_words(rc)
        assert len(got) == len(s) // 16 + 3
        assert np.array_equal(got, want), (q, len(s), [hex(x) for x in got], [hex(x) for x in want])
    assert np.array_equal(sc.fetch_seq(n + n - 2), seqs[n - 2])  # the palindrome
    sc.upload_seqs(seqs[:3])
    assert sc.strands == 1 and sc.nseqs == 3
    sc.close()


def hit_fields(h):
    return [bits(h[f]).tolist() if f.endswith("loglik") else h[f].tolist()
            for f in ("seq_idx", "profile_idx", "null_loglik", "alt_loglik")]


SAME_BITS_CASES = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 4)]  # (precision, dcp_scan_params.kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("multi_hits", [False, True])
@pytest.mark.parametrize("precision,kernel", SAME_BITS_CASES)
def test_same_bits_as_a_hand_doubled_batch(dcp, precision, kernel, multi_hits):
    """Scan A: n queries + add_reverse_strand.  Scan B: the 2n sequences through upload_seqs.  (One case per kernel
    and multi_hits value, both hmmer3_compat values and both thresholds in each: the 10 007-nt query bounds a scan.)"""
    profs, seqs = world(dcp, precision)
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    a.upload_seqs(seqs)
    a.add_reverse_strand()
    b.upload_seqs(seqs + [np_revcomp(s) for s in seqs])
    assert a.nseqs == b.nseqs == 2 * len(seqs)
    assert a.cells == b.cells and a.algorithmic_bytes == b.algorithmic_bytes
    for h3 in (False, True):
        for thr in (10.0, 0.0):
            a.scan(multi_hits, h3, thr, kernel=kernel)
            b.scan(multi_hits, h3, thr, kernel=kernel)
            where = (precision, kernel, multi_hits, h3, thr)
            for x, y in zip(a.scores(), b.scores()):
                assert np.array_equal(bits(x), bits(y)), where
            assert hit_fields(a.hits()) == hit_fields(b.hits()), where
            assert a.last_scan_redo_pairs == b.last_scan_redo_pairs, where
            assert a.last_scan_kernel == b.last_scan_kernel == kernel, where
            if kernel == dcp.KERNEL_QLANE64:
                assert a.last_scan_query_plan == b.last_scan_query_plan, where
    a.close()
    b.close()


# ---- a hit on the minus strand only ------------------------------------------------------------------------------

PLANT_SEED = {32: 4100, 64: 4200}  # both premises hold for every planted pair of either precision (checked on the CPU)
PLANT_M = (40, 130, 300)


def planted_world(dcp, oracle, precision):
    """Pfam-like profiles, their oracle twins, and per profile a query with a planted copy of it (from the profile's
    most likely codons, as the edge tests plant them)."""
    rng = np.random.default_rng(PLANT_SEED[precision])
    params = [pfam_like_params(rng, M) for M in PLANT_M]
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
    profs = [dcp.ProteinProfile.from_params(*prm, cfg, f"PLANT{i}", precision=precision) for i, prm in enumerate(params)]
    oprofs = [oracle.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01) for prm in params]
    orig = [planted_query(rng, oprofs[p], M, flank=12) for p, M in enumerate(PLANT_M)]
    noise = [rng.integers(0, 4, L, dtype=np.uint8) for L in (1, 17, 90, 400)]
    return profs, oprofs, orig, noise


def oracle_lrt(oracle, oprofs, seqs):
    _, on, oa = oracle.scan(oprofs, [bytes(s) for s in seqs], True, False, 10.0, 1, 1)
    return -2.0 * (on.astype(np.float64) - oa.astype(np.float64))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_premises_of_the_minus_strand_hit_on_the_oracle(dcp, oracle32, oracle64, precision):
    """CPU: the original query hits its profile, its reverse complement does not -- for every planted pair of the
    seeds kept above."""
    oracle = oracle64 if precision == 64 else oracle32
    _, oprofs, orig, _ = planted_world(dcp, oracle, precision)
    fwd = oracle_lrt(oracle, oprofs, orig)
    rev = oracle_lrt(oracle, oprofs, [np_revcomp(s) for s in orig])
    for p in range(len(PLANT_M)):
        assert fwd[p, p] >= 10.0, (p, fwd[p, p])
        assert not rev[p, p] >= 10.0, (p, rev[p, p])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hit_on_the_minus_strand_only(dcp, oracle32, oracle64, precision):
    oracle = oracle64 if precision == 64 else oracle32
    profs, oprofs, orig, noise = planted_world(dcp, oracle, precision)
    nplant = len(orig)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    # the original queries scanned directly: the bits, paths and rows the minus strand must reproduce
    sc.upload_seqs(orig + noise)
    sc.scan(True, False, 10.0)
    want = {(int(h["seq_idx"]), int(h["profile_idx"])): h.copy() for h in sc.hits()}
    assert all((p, p) in want for p in range(nplant))  # premise 1 on the device
    own = np.array([want[(p, p)] for p in range(nplant)])
    want_paths, _ = sc.trace_paths(own, True, False)
    want_rows = [profs[p].prod_row(orig[p], want_paths[p], 3, 77, own[p]["alt_loglik"], own[p]["null_loglik"])
                 for p in range(nplant)]
    # the batch as a caller holds it: the other strand of every read
    fwd = [np_revcomp(s) for s in orig] + noise
    n = len(fwd)
    sc.upload_seqs(fwd)
    sc.scan(True, False, 10.0)
    plain = {(int(h["seq_idx"]), int(h["profile_idx"])) for h in sc.hits()}
    assert not any((p, p) in plain for p in range(nplant))  # premise 2 on the device
    sc.add_reverse_strand()
    for kernel in kernels_of(dcp, precision):
        sc.scan(True, False, 10.0, kernel=kernel)
        got = {(int(h["seq_idx"]), int(h["profile_idx"])): h.copy() for h in sc.hits()}
        assert {k for k in got if k[0] < n} == plain
        for p in range(nplant):
            h = got[(n + p, p)]
            assert bits(h["null_loglik"]) == bits(own[p]["null_loglik"]), (kernel, p)
            assert bits(h["alt_loglik"]) == bits(own[p]["alt_loglik"]), (kernel, p)
    minus = np.array([got[(n + p, p)] for p in range(nplant)])
    paths, alt = sc.trace_paths(minus, True, False)
    for p in range(nplant):
        assert np.array_equal(paths[p], want_paths[p]), p
        assert bits(alt[p]) == bits(own[p]["alt_loglik"])
        seq = sc.fetch_seq(n + p)
        assert np.array_equal(seq, orig[p])
        assert profs[p].prod_row(seq, paths[p], 3, 77, minus[p]["alt_loglik"], minus[p]["null_loglik"]) == want_rows[p]
    sc.close()


# ---- ranges and mixed lengths ------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ranged_scans_of_the_doubled_batch(dcp, precision):
    profs, seqs = world(dcp, precision)
    n = len(seqs)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()
    keep_all = -1e30  # every pair with a finite ratio is a hit: the lists compared are as long as they can be
    sc.scan(True, False, keep_all)
    fn, fa = sc.scores()
    fh = sc.hits()
    for kernel in kernels_of(dcp, precision):
        for q0, q1 in ((n, 2 * n), (n - 3, n + 3), (0, n)):
            sc.scan(True, False, keep_all, q_range=(q0, q1), kernel=kernel)
            gn, ga = sc.scores()
            assert np.array_equal(bits(gn[q0:q1]), bits(fn[q0:q1])), (kernel, q0, q1)
            assert np.array_equal(bits(ga[q0:q1]), bits(fa[q0:q1])), (kernel, q0, q1)
            sel = fh[(fh["seq_idx"] >= q0) & (fh["seq_idx"] < q1)]
            assert hit_fields(sc.hits()) == hit_fields(sel), (kernel, q0, q1)
            assert len(sel) > 0
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mixed_lengths_doubled_through_the_query_lane_kernels(dcp, precision):
    """300 queries of 1 nt .. 12 kbp, doubled on the device: sequences of every length share the word kernel's grid
    (3 to 753 words each), and the 600 resident ones run through the packed query-lane kernel -- kernel 3 on the float
    DB, kernel 4 on the double one -- to the row sweep's scores as integers."""
    profs, _ = world(dcp, precision)
    rng = np.random.default_rng(1200 + precision)
    lens = np.exp(rng.uniform(0.0, np.log(12000.0), 300)).astype(np.int64)
    lens[11], lens[250] = 1, 12000
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()
    assert sc.nseqs == 600
    for q in (0, 11, 250, 299):
        assert np.array_equal(sc.fetch_seq(300 + q), np_revcomp(seqs[q])), q
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    rn, ra = sc.scores()
    rh = sc.hits()
    lane = dcp.KERNEL_QLANE64 if precision == 64 else dcp.KERNEL_QLANE2
    sc.scan(True, False, 10.0, kernel=lane)
    assert sc.last_scan_kernel == lane
    gn, ga = sc.scores()
    assert np.array_equal(bits(gn), bits(rn)) and np.array_equal(bits(ga), bits(ra))
    assert hit_fields(sc.hits()) == hit_fields(rh)
    sc.close()


# ---- contract ----------------------------------------------------------------------------------------------------


def refused(dcp, sc, call, rc=None):
    with pytest.raises(dcp.DcpError) as e:
        call()
    assert e.value.rc == (dcp.RC_EINVAL if rc is None else rc)
    assert len(str(e.value)) > len("RC_EINVAL: ")  # a message was set


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_contract(dcp, precision):
    profs, seqs = world(dcp, precision)
    seqs = seqs[:12]
    n = len(seqs)
    sc = dcp.Scanner(0)
    refused(dcp, sc, sc.add_reverse_strand)  # before any upload, and with no DB resident
    assert sc.strands == 0 and sc.nseqs == 0
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()  # no DB resident: sequences only
    refused(dcp, sc, sc.add_reverse_strand)  # twice
    assert sc.strands == 2 and sc.nseqs == 2 * n  # the context is as it was
    sc.upload_db(profs)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    want = [bits(x).copy() for x in sc.scores()]
    # explicit transitions in force: refused, in the precision of the DB
    derived = (dcp.xtrans64 if precision == 64 else dcp.xtrans)
    rows = lambda ss: np.stack([derived(len(s), True, False) for s in ss])
    sc.upload_seqs(seqs)
    sc.set_xtrans(rows(seqs))
    refused(dcp, sc, sc.add_reverse_strand)
    assert sc.strands == 1 and sc.nseqs == n
    sc.upload_seqs(seqs)  # the next upload lifts them
    sc.add_reverse_strand()
    refused(dcp, sc, lambda: sc.set_xtrans(rows(seqs)))  # n rows for 2n sequences
    sc.set_xtrans(rows(seqs + seqs))  # 2n rows: accepted, and the flag-derived rows reproduce the flag-derived scan
    sc.scan(False, True, 10.0, kernel=dcp.KERNEL_ROWSWEEP)  # the flags are ignored
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    # fetch_seq
    refused(dcp, sc, lambda: sc.fetch_seq(2 * n))
    ln = C.c_uint(0)
    buf = np.zeros(64, np.uint8)
    q = n + 7  # 17 symbols
    assert len(seqs[7]) == 17
    rc = sc._lib.dcp_gpu_seqs_fetch(sc._c, q, buf.ctypes.data, 16, C.byref(ln))
    assert rc == dcp.RC_ENOMEM and ln.value == 17 and not buf.any()
    assert sc._lib.dcp_gpu_last_error(sc._c)
    rc = sc._lib.dcp_gpu_seqs_fetch(sc._c, q, buf.ctypes.data, 17, C.byref(ln))
    assert rc == 0 and ln.value == 17 and np.array_equal(buf[:17], np_revcomp(seqs[7]))
    # still usable
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y[:n])
    sc.close()
