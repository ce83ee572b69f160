"""The double build (the reference's IMM_DOUBLE_PRECISION) from the profile to the hits.

CPU: the f64 profile parts and special transitions against the oracle's double build (bit-exact: both are
imm's log-domain chains on the same C library), and the float profiles' bytes unchanged.
GPU: goldens G1-G3 through the device, random f64 profiles against the oracle's f64 Viterbi on every pair,
the hit set against the oracle's LRT filter, and the errors of mixing float and double."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM


def cfg64(dcp, entry, eps):
    # the reference's cfg literals are floats (protein_cfg(..., 0.1f)); its double build widens them
    return dcp.ProteinCfg(entry, float(np.float32(eps)))


# ---- CPU -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("entry", [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY])
@pytest.mark.parametrize("M", [2, 3, 100, 4096])
def test_sample64_parts_equal_oracle64(dcp, oracle64, entry, M):
    """Exact: same operations in the same order, same libm."""
    for seed in (1, 2, 7):
        p = dcp.ProteinProfile.sample(seed, M, cfg64(dcp, entry, 0.01), precision=64)
        assert p.precision == 64 and p.core_size == M
        t8, nd, idd, md = p.parts64()
        op = oracle64.sample(seed, M, entry, 0.01)
        ond, oid, omd = op.dists()
        assert np.array_equal(t8, op.export()[0])
        assert np.array_equal(nd, ond)
        assert np.array_equal(idd, oid)
        assert np.array_equal(md, omd)
        # the float views are the same values rounded once
        assert np.array_equal(p.trans8, t8.astype(np.float32))
        assert np.array_equal(p.match_dist, md.astype(np.float32))


def random_params(rng, M, delete_heavy=False):
    def norm(x):
        return x - np.logaddexp.reduce(x, axis=-1, keepdims=True)

    null = norm(np.log(rng.random(20)))
    match = norm(np.log(rng.random((M, 20))))
    tr = np.log(rng.random((M + 1, 7)))
    if delete_heavy:
        tr[:, 2] += 4.0  # MD
        tr[:, 6] += 4.0  # DD
    tr[0, 6] = -np.inf
    tr[M, 2] = tr[M, 6] = -np.inf
    return null, match, norm(tr)


@pytest.mark.parametrize("M", [1, 2, 3, 100, 4096])
def test_new64_parts_equal_oracle64(dcp, oracle64, M):
    rng = np.random.default_rng(M)
    for entry in (ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY):
        null, match, tr = random_params(rng, M)
        p = dcp.ProteinProfile.from_params(null, match, tr, cfg64(dcp, entry, 0.01), precision=64)
        op = oracle64.new(null, match, tr, entry, 0.01)
        t8, nd, idd, md = p.parts64()
        ond, oid, omd = op.dists()
        assert np.array_equal(t8, op.export()[0])
        assert np.array_equal(nd, ond) and np.array_equal(idd, oid) and np.array_equal(md, omd)


def test_xtrans64_equals_oracle64(dcp, oracle64):
    for mh in (False, True):
        for h3 in (False, True):
            for L in (1, 2, 3, 5, 32, 300, 10000, 123457):
                rc, ref = oracle64.xtrans(L, mh, h3)
                assert rc == 0
                assert np.array_equal(dcp.xtrans64(L, mh, h3), ref), (L, mh, h3)
    with pytest.raises(dcp.DcpError):
        dcp.xtrans64(0)


def test_float_profile_has_no_double_parts(dcp):
    p = dcp.ProteinProfile.sample(3, 10)
    assert p.precision == 32
    with pytest.raises(dcp.DcpError):
        p.parts64()
    with pytest.raises(dcp.DcpError):
        dcp.ProteinProfile.sample(3, 10, precision=16)


# sha256 of the float profiles' parts (trans8, null, insert, match dists) as the library built them before the
# double build existed; a float profile must not change by a bit
FLOAT_PARTS_SHA256 = {  # (seed, core_size, entry_dist, epsilon)
    (1, 2, 1, 0.1): "c13b5553ac9d21c5c92837020e7db73b2e757f3b58728136c7010c13be4a5c1e",
    (1, 2, 2, 0.1): "56fff2cad1fcc09564ef582ab2c88613991ea8519dda128e441556338cf17454",
    (7, 100, 2, 0.01): "344195bc09c0f6633ea723044b4ceac3159ad396bee8c96dc41939ec15c1386a",
    (11, 4096, 1, 0.01): "c73b694ea75858eed5bdf70f1e6489231ffa26a369faafa37d05f786a58b6d7a",
    (3, 513, 2, 0.5): "2be3b8b8930d39beb20fd67b588e83210d98d722810ea3ed09c7b588c801ea43",
}


def float_parts_digest(p):
    h = hashlib.sha256()
    for a in (p.trans8, p.null_dist, p.insert_dist, p.match_dist):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def test_float_profiles_unchanged(dcp):
    for (seed, M, entry, eps), digest in FLOAT_PARTS_SHA256.items():
        assert float_parts_digest(dcp.ProteinProfile.sample(seed, M, dcp.ProteinCfg(entry, eps))) == digest


# ---- GPU -------------------------------------------------------------------------------------------------------

SEQ = "ATGAAACGCATTAGCACCACCATTACCACCAC"  # test/protein_profile.c of the reference
NULL_LL = -48.9272687711
ALT_LL = {ENTRY_DIST_UNIFORM: -55.59428153448, ENTRY_DIST_OCCUPANCY: -54.35543421312}


@pytest.mark.gpu
def test_goldens_through_the_device(dcp):
    sc = dcp.Scanner(0)
    for entry in (ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY):
        sc.upload_db([dcp.ProteinProfile.sample(1, 2, cfg64(dcp, entry, 0.1), precision=64)])
        assert sc.precision == 64
        sc.upload_seqs([SEQ])
        for kernel in (dcp.KERNEL_AUTO, dcp.KERNEL_ROWSWEEP):
            sc.scan(True, False, 10.0, kernel=kernel)
            nl, al = sc.scores()
            assert nl.dtype == np.float64 and al.dtype == np.float64
            assert abs(nl[0, 0] - NULL_LL) < 1e-10
            assert abs(al[0, 0] - ALT_LL[entry]) < 1e-10
    sc.close()


def oracle_scores(oracle64, oprofs, seqs, mh, h3):
    _, on, oa = oracle64.scan(oprofs, [bytes(s) for s in seqs], mh, h3, 10.0, 16, 1)
    return np.asarray(on, np.float64), np.asarray(oa, np.float64)


def assert_scores_match(got, ref):
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf])
    err = np.abs(got[~inf] - ref[~inf]) / np.maximum(1.0, np.abs(ref[~inf]))
    assert err.max(initial=0.0) <= 1e-12, err.max()


@pytest.mark.gpu
def test_random_profiles_against_oracle64(dcp, oracle64):
    rng = np.random.default_rng(64)
    Ms = [1, 2, 63, 64, 65, 128, 512, 513, 1024, 4096]
    Ls = [1, 2, 3, 4, 5, 100, 1000, 10000]
    profs, oprofs = [], []
    for i, M in enumerate(Ms + [300, 700]):  # the last two: delete-heavy (most of the mass on MD / DD)
        null, match, tr = random_params(rng, M, delete_heavy=i >= len(Ms))
        entry = (ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2]
        profs.append(dcp.ProteinProfile.from_params(null, match, tr, cfg64(dcp, entry, 0.01), precision=64))
        oprofs.append(oracle64.new(null, match, tr, entry, 0.01))
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in Ls]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    for mh in (False, True):
        for h3 in (False, True):
            sc.scan(mh, h3, 10.0)
            gn, ga = sc.scores()
            on, oa = oracle_scores(oracle64, oprofs, seqs, mh, h3)
            assert_scores_match(gn, on)
            assert_scores_match(ga, oa)
    sc.close()


@pytest.mark.gpu
def test_hits_equal_oracle64_lrt_filter(dcp, oracle64):
    """Profiles that favour methionine (ATG, its only codon) against sequences with and without ATG runs: the
    thresholds 10 and 0 both separate hits from non-hits."""
    rng = np.random.default_rng(7)
    profs, oprofs = [], []
    for M in rng.integers(1, 700, 24):
        null, match, tr = random_params(rng, int(M))
        match[:, 10] += 3.0  # 'M' of ACDEFGHIKLMNPQRSTVWY
        match -= np.logaddexp.reduce(match, axis=-1, keepdims=True)
        profs.append(dcp.ProteinProfile.from_params(null, match, tr, cfg64(dcp, ENTRY_DIST_OCCUPANCY, 0.01),
                                                    precision=64))
        oprofs.append(oracle64.new(null, match, tr, ENTRY_DIST_OCCUPANCY, 0.01))
    seqs = []
    for i in range(30):
        flank = [rng.integers(0, 4, int(rng.integers(1, 200)), dtype=np.uint8) for _ in range(2)]
        run = np.tile(np.array([0, 3, 2], np.uint8), int(rng.integers(0, 40)) if i % 3 else 0)  # ATG x n
        seqs.append(np.concatenate([flank[0], run, flank[1]]))
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    on, oa = oracle_scores(oracle64, oprofs, seqs, True, False)
    lrt = -2 * (on - oa)
    for thr in (10.0, 0.0):
        sc.scan(True, False, thr, keep_scores=False)
        h = sc.hits()
        assert h.dtype == dcp.HIT64_DTYPE
        keep = np.isfinite(lrt) & (lrt >= thr)
        assert 0 < int(keep.sum()) < keep.size
        want = [(int(q), int(p)) for q, p in zip(*np.nonzero(keep))]
        got = list(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist()))
        assert got == want
        q, p = h["seq_idx"], h["profile_idx"]
        assert_scores_match(h["null_loglik"], on[q, p])
        assert_scores_match(h["alt_loglik"], oa[q, p])
    sc.close()


@pytest.mark.gpu
def test_errors_of_mixing_precisions(dcp):
    lib = dcp.lib
    p32 = dcp.ProteinProfile.sample(1, 20)
    p64 = dcp.ProteinProfile.sample(1, 20, precision=64)
    sc = dcp.Scanner(0)
    with pytest.raises(dcp.DcpError):
        sc.upload_db([p32, p64])
    arr = (C.c_void_p * 1)(p32._h)
    assert lib.dcp_gpu_db_upload64(sc._c, arr, 1) == dcp.RC_EINVAL
    arr = (C.c_void_p * 1)(p64._h)
    assert lib.dcp_gpu_db_upload(sc._c, arr, 1, 0) == dcp.RC_EINVAL
    sc.upload_db([p64])
    with pytest.raises(dcp.DcpError):
        sc.upload_seqs([""])
    sc.upload_seqs(["ACGTACGTAC", "GATTACA"])
    for kernel in (dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2):
        with pytest.raises(dcp.DcpError):
            sc.scan(kernel=kernel)
    sc.scan(True, False, -1e300)
    # a float fetch after a double scan is refused, never rounded
    nl = np.zeros((2, 1), np.float32)
    assert lib.dcp_gpu_fetch_scores(sc._c, nl.ctypes.data, nl.ctypes.data) == dcp.RC_EINVAL
    assert b"double" in lib.dcp_gpu_last_error(sc._c)
    hb = np.zeros(4, dcp.HIT_DTYPE)
    n = C.c_uint(0)
    assert lib.dcp_gpu_fetch_hits(sc._c, hb.ctypes.data, 4, C.byref(n)) == dcp.RC_EINVAL
    assert len(sc.hits()) == 2
    # and the reverse: a double fetch after a float scan
    sc.upload_db([p32])
    assert sc.precision == 32
    sc.upload_seqs(["ACGTACGTAC", "GATTACA"])
    sc.scan(True, False, 10.0)
    nl64 = np.zeros((2, 1), np.float64)
    assert lib.dcp_gpu_fetch_scores64(sc._c, nl64.ctypes.data, nl64.ctypes.data) == dcp.RC_EINVAL
    hb64 = np.zeros(4, dcp.HIT64_DTYPE)
    assert lib.dcp_gpu_fetch_hits64(sc._c, hb64.ctypes.data, 4, C.byref(n)) == dcp.RC_EINVAL
    assert sc.scores()[0].dtype == np.float32
    sc.close()
