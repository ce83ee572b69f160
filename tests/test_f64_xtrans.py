"""Explicit special transitions in double (dcp_gpu_seqs_set_xtrans64) on a double DB, in bits.

Every comparison is made as uint64, with no tolerance.

  1. explicit equals derived: the rows dcp_xtrans64(L, multi_hits, hmmer3_compat) given per query reproduce the
     flag-derived scan -- null / alt scores, every dcp_hit64 field, trace_paths step for step -- under kernels 1 and 4
     and all four flag combinations, while the scan itself is asked with the OPPOSITE flags (they are ignored);
  2. transitions no flags produce: the LOG1 defaults (all zero) and seeded random rows with -inf entries, E -> B and
     E -> J finite while the scan says multi_hits = 0: kernels 1 and 4 equal the oracle's f64 recursion on the DB's own
     tables with that row, paths equal its walk; planted multi-copy queries come back through kernel 4's redo lists;
  3. the refusals, and a new sequence upload that restores the derived rows.

The bounds are the issue's: bit equality, with the oracle's double build (orc_dp_tables / orc_dp_tables_path on the
tables read back from the device) as the reference."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM
from test_f64_bits import Tables64, u64
from test_f64_edges import FLAGS, make_profiles, planted_family
from test_f64_qlane import same_hits
from test_f64_scan import random_params

pytestmark = pytest.mark.gpu

EDGE_M = [1, 64, 65, 128, 129, 256, 257, 1024, 4096]  # the launch groups' edges
EDGE_L = list(range(1, 34)) + [100, 1000]
NINF = -np.inf


def kernels(dcp):
    return (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE64)


def scan_all(sc, kernel, mh, h3, thr):
    sc.scan(mh, h3, thr, kernel=kernel)
    assert sc.last_scan_kernel == kernel
    gn, ga = sc.scores()
    return gn, ga, sc.hits()


def same_paths(a, b):
    return len(a) == len(b) and all(np.array_equal(x["state_id"], y["state_id"]) and
                                    np.array_equal(x["seqlen"], y["seqlen"]) for x, y in zip(a, b))


def test_explicit_equals_derived(dcp, oracle64):
    """A mixed-length batch against core sizes on the launch groups' edges: the explicit rows of the flags give the
    flag-derived scan's bits, hits and paths, whatever flags the scan and the trace themselves are given."""
    rng = np.random.default_rng(6413)
    sizes = [EDGE_M[i] for i in rng.permutation(len(EDGE_M))]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(len(sizes))])
    lens = [int(L) for L in rng.permutation(EDGE_L)]
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in lens]
    thr = -1e300  # every pair with a finite LRT is a hit, and is traced
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    for mh, h3 in FLAGS:
        sc.upload_seqs(seqs)
        derived = {}
        for k in kernels(dcp):
            gn, ga, h = scan_all(sc, k, mh, h3, thr)
            assert len(h) > len(seqs) * len(profs) // 2
            paths, alt = sc.trace_paths(h, mh, h3)
            assert np.array_equal(u64(alt), u64(h["alt_loglik"]))
            derived[k] = (gn, ga, h, paths)
        sc.set_xtrans(np.stack([dcp.xtrans64(L, mh, h3) for L in lens]))
        for k in kernels(dcp):
            gn, ga, h = scan_all(sc, k, not mh, not h3, thr)
            rn, ra, rh, rpaths = derived[k]
            assert np.array_equal(u64(gn), u64(rn)) and np.array_equal(u64(ga), u64(ra)), (k, mh, h3)
            assert same_hits(h, rh), (k, mh, h3, len(h), len(rh))
            paths, alt = sc.trace_paths(h, not mh, not h3)
            assert np.array_equal(u64(alt), u64(h["alt_loglik"]))
            assert same_paths(paths, rpaths), (k, mh, h3)
        # both kernels agree with each other, too
        assert same_hits(derived[dcp.KERNEL_ROWSWEEP][2], derived[dcp.KERNEL_QLANE64][2])
    sc.close()


def random_rows(rng, n):
    """rows of 13 log-transitions in [-4, 0] with about a fifth of the entries -inf; E -> B and E -> J stay finite"""
    xt = -4.0 * rng.random((n, 13))
    xt[rng.random(xt.shape) < 0.2] = NINF
    xt[:, 9] = -3.0 * rng.random(n)   # EB
    xt[:, 10] = -3.0 * rng.random(n)  # EJ
    return xt


def check_rows(dcp, oracle64, sc, tabs, seqs, xt, thr, want_redo=None):
    """with the rows xt resident: kernels 1 and 4 under multi_hits = 0 against the oracle's f64 recursion on the
    device's tables with each query's row -- scores, the LRT filter, every hit field -- and the paths of every pair
    with a finite alt score against the oracle's walk.  Returns kernel 4's redo pairs."""
    nq, nprof = len(seqs), sc.nprofiles
    ref_n, ref_a = np.zeros((nq, nprof)), np.zeros((nq, nprof))
    walks = {}
    for q in range(nq):
        for p in range(nprof):
            t8, em, ei, en = tabs.t[p]
            nl, al, apath, _ = oracle64.dp_tables_path(t8, em, ei, en, xt[q], bytes(seqs[q]))
            rc, nl2, al2 = oracle64.dp_tables(t8, em, ei, en, xt[q], bytes(seqs[q]))
            assert rc == 0 and u64(nl) == u64(nl2) and u64(al) == u64(al2)
            ref_n[q, p], ref_a[q, p] = nl, al
            walks[(q, p)] = apath
    with np.errstate(invalid="ignore"):
        lrt = -2 * (ref_n - ref_a)
        keep = np.isfinite(lrt) & (lrt >= thr)
    want = sorted((int(q), int(p)) for q, p in zip(*np.nonzero(keep)))
    redo = None
    for k in kernels(dcp):
        gn, ga, h = scan_all(sc, k, False, False, thr)
        if k == dcp.KERNEL_QLANE64:
            redo = sc.last_scan_redo_pairs
        bad = np.argwhere((u64(gn) != u64(ref_n)) | (u64(ga) != u64(ref_a)))
        assert len(bad) == 0, (k, len(bad), [(int(q), int(p), gn[q, p], ref_n[q, p], ga[q, p], ref_a[q, p])
                                             for q, p in bad[:5]])
        assert list(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist())) == want, k
        assert np.array_equal(u64(h["null_loglik"]), u64(ref_n[h["seq_idx"], h["profile_idx"]]))
        assert np.array_equal(u64(h["alt_loglik"]), u64(ref_a[h["seq_idx"], h["profile_idx"]]))
        pairs = [(q, p) for q in range(nq) for p in range(nprof) if np.isfinite(ref_a[q, p])]
        assert len(pairs) > nq * nprof // 4
        recs = np.array([(q, p, ref_n[q, p], ref_a[q, p]) for q, p in pairs], dcp.HIT64_DTYPE)
        paths, alt = sc.trace_paths(recs, False, False)
        assert np.array_equal(u64(alt), u64(recs["alt_loglik"]))
        for (q, p), path in zip(pairs, paths):
            st, ln = walks[(q, p)]
            assert np.array_equal(path["state_id"], st) and np.array_equal(path["seqlen"], ln), (k, q, p)
            assert int(path["seqlen"].sum()) == len(seqs[q])
    if want_redo is not None:
        assert (redo > 0) == want_redo, redo
    return redo


def test_transitions_no_flags_produce(dcp, oracle64):
    """LOG1 rows (all zero: a profile that never saw protein_profile_setup) and random rows with -inf entries, both
    with E -> B / E -> J finite under a scan that says multi_hits = 0."""
    rng = np.random.default_rng(1364)
    sizes = [1, 5, 64, 65, 129, 257, 300, 600]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [(ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM)[i % 2] for i in range(len(sizes))])
    lens = [1, 2, 3, 5, 6, 16, 17, 33, 100, 257, 400]
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in lens]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    sc.set_xtrans(np.zeros((len(seqs), 13)))
    check_rows(dcp, oracle64, sc, tabs, seqs, np.zeros((len(seqs), 13)), thr=0.0)
    for seed in (1, 2, 3):
        xt = random_rows(np.random.default_rng(seed), len(seqs))
        sc.set_xtrans(xt)
        check_rows(dcp, oracle64, sc, tabs, seqs, xt, thr=(-20.0, 0.0, 10.0)[seed - 1])
    sc.close()


def test_planted_copies_come_back_through_the_redo_lists(dcp, oracle64):
    """Planted multi-copy queries (test_f64_qlane.test_redo_path's kind) with the multi-hit rows given explicitly and
    multi_hits = 0 in the scan: the best paths re-enter B, so kernel 4 must keep its redo lists and launches --
    last_scan_redo_pairs > 0 -- and give the oracle's bits; with the uni-hit rows given, nothing is redone."""
    fams = [planted_family(oracle64, M) for M in (30, 100, 257)]
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * len(fams))
    seqs = [s for f in fams for k, _, s in f[2] if k in (1, 2, 3)]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    xt = np.stack([dcp.xtrans64(len(s), True, False) for s in seqs])
    sc.set_xtrans(xt)
    check_rows(dcp, oracle64, sc, tabs, seqs, xt, thr=10.0, want_redo=True)
    xt = np.stack([dcp.xtrans64(len(s), False, False) for s in seqs])
    sc.set_xtrans(xt)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE64)  # the flag is ignored: these rows have no feedback
    assert sc.last_scan_redo_pairs == 0
    sc.close()


def test_refusals(dcp):
    lib = dcp.lib
    seqs = ["ACGTACGTACGTAAAGGG", "GATTACA"]
    lens = [len(s) for s in seqs]
    rows = np.stack([dcp.xtrans64(L, True, False) for L in lens])

    def rc_of(f):
        with pytest.raises(dcp.DcpError) as e:
            f()
        return e.value.rc

    sc = dcp.Scanner(0)
    sc.upload_db([dcp.ProteinProfile.sample(3, 300, precision=64), dcp.ProteinProfile.sample(4, 20, precision=64)])
    # no sequences resident yet
    assert lib.dcp_gpu_seqs_set_xtrans64(sc._c, rows.ctypes.data, 2) == dcp.RC_EINVAL
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e300)
    ref = sc.scores()
    ref_hits = sc.hits()
    # a NaN, by its bit pattern (quiet, signalling, negative), anywhere
    for bits in (0x7ff8000000000000, 0x7ff0000000000001, 0xfff8000000000000):
        bad = rows.copy()
        bad.view(np.uint64)[1, 12] = bits
        assert lib.dcp_gpu_seqs_set_xtrans64(sc._c, bad.ctypes.data, 2) == dcp.RC_EINVAL
    # infinities are values
    inf = rows.copy()
    inf[0, 9] = NINF
    assert lib.dcp_gpu_seqs_set_xtrans64(sc._c, inf.ctypes.data, 2) == dcp.RC_OK
    # a wrong nseqs, a null pointer
    for n in (0, 1, 3):
        assert lib.dcp_gpu_seqs_set_xtrans64(sc._c, rows.ctypes.data, n) == dcp.RC_EINVAL
    assert lib.dcp_gpu_seqs_set_xtrans64(sc._c, None, 2) == dcp.RC_EINVAL
    assert rc_of(lambda: sc.set_xtrans64(rows[:1])) == dcp.RC_EINVAL
    # the refused calls left the last accepted rows in force; a new upload restores the derived ones
    sc.upload_seqs(seqs)
    for k in kernels(dcp):
        sc.scan(True, False, -1e300, kernel=k)
        n, a = sc.scores()
        assert np.array_equal(u64(n), u64(ref[0])) and np.array_equal(u64(a), u64(ref[1]))
    # explicit rows, then an upload: derived again (the uni-hit rows would change the scores)
    sc.set_xtrans(np.stack([dcp.xtrans64(L, False, False) for L in lens]))
    sc.scan(True, False, -1e300)
    n, a = sc.scores()
    assert not np.array_equal(u64(a), u64(ref[1]))
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e300)
    n, a = sc.scores()
    assert np.array_equal(u64(n), u64(ref[0])) and np.array_equal(u64(a), u64(ref[1]))
    assert same_hits(sc.hits(), ref_hits)
    # float transitions on a double DB: still DCP_EINVAL at the scan, kernel 1 and 4
    sc.set_xtrans(np.tile(dcp.xtrans(7, True, False), (2, 1)))
    for k in (dcp.KERNEL_AUTO,) + kernels(dcp):
        assert rc_of(lambda: sc.scan(True, False, 10.0, kernel=k)) == dcp.RC_EINVAL
    # the last set holds: double rows after float ones are taken
    sc.set_xtrans(rows)
    sc.scan(False, True, -1e300)
    n, a = sc.scores()
    assert np.array_equal(u64(n), u64(ref[0])) and np.array_equal(u64(a), u64(ref[1]))
    sc.close()

    # double transitions on a float DB: DCP_EINVAL at the scan (every kernel) and at the trace, with a message
    sc = dcp.Scanner(0)
    sc.upload_db([dcp.ProteinProfile.sample(3, 300), dcp.ProteinProfile.sample(4, 20)])
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e30)
    h = sc.hits()
    fn, fa = sc.scores()
    assert len(h) > 0
    sc.set_xtrans64(rows)
    for k in (dcp.KERNEL_AUTO, dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2):
        assert rc_of(lambda: sc.scan(True, False, 10.0, kernel=k)) == dcp.RC_EINVAL
        assert b"double" in lib.dcp_gpu_last_error(sc._c)
    assert rc_of(lambda: sc.trace_paths(h)) == dcp.RC_EINVAL
    assert b"double" in lib.dcp_gpu_last_error(sc._c)
    # a float64 array through set_xtrans on a float DB is taken as float, as before
    sc.set_xtrans(np.stack([dcp.xtrans(L, True, False) for L in lens]).astype(np.float64))
    sc.scan(False, True, -1e30)
    n, a = sc.scores()
    assert np.array_equal(n.view(np.uint32), fn.view(np.uint32)) and np.array_equal(a.view(np.uint32), fa.view(np.uint32))
    # and an upload clears the double rows
    sc.set_xtrans64(rows)
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e30)
    n, a = sc.scores()
    assert np.array_equal(n.view(np.uint32), fn.view(np.uint32)) and np.array_equal(a.view(np.uint32), fa.view(np.uint32))
    sc.trace_paths(sc.hits())
    sc.close()
