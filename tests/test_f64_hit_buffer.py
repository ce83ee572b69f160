"""The double scan's hit records in caller-owned device memory (dcp_gpu_set_hit_buffer64 / dcp_gpu_hit_buffer64).

Every path of a scan of a double DB writes `struct dcp_hit64` records behind `if (h < hit_cap)`: viterbi64_kernel in
grid mode (kernel 0 and 1), viterbi64_qlane_kernel (kernel 4), the row sweep's pair-list launches behind kernel 4, a
ranged scan, and the repeat with the row sweep after kernel 4's redo lists overflowed.  Each is scanned here into a
torch tensor of cap + 8 rows of 6 int32 words filled with 0xA5A5A5A5, of which the library is told `cap`: the counter
counts every hit, nothing is written at or behind row `cap`, and what is held are the records the context's own buffer
gives, compared as bits.  The DB is twelve double profiles on the f64 launch groups' and the segment's edges, the batch
about a hundred queries with a planted hit in every launch group."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the product's library: both bring a HIP runtime, and torch must see the device too

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_f64_edges import make_profiles, planted_family
from test_gpu_parity import pfam_like_params, planted_query

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
FILL_I32 = int(np.array(FILL, np.uint32).view(np.int32))
GUARD = 8
SIZES = [1, 5, 40, 64, 65, 128, 129, 200, 256, 257, 300, 513]
PLANTED = {3: 3, 17: 5, 30: 8, 44: 9, 58: 11, 71: 2, 72: 10}  # query -> profile: every launch group (64, 128, 256, > 256)


def words_of(records):
    """[n, 6] uint32 words of HIT64_DTYPE records"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 6)


def same_bits(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and np.array_equal(words_of(a), words_of(b))


def by_key(records):
    return records[np.lexsort((records["profile_idx"], records["seq_idx"]))]


def build_world(dcp, oracle64, seed=64, nq=90, planted=PLANTED):
    rng = np.random.default_rng(seed)
    params = [pfam_like_params(rng, M) for M in SIZES]
    profs, oprofs = make_profiles(dcp, oracle64, params, [ENTRY_DIST_OCCUPANCY] * len(SIZES))
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(30, 201, nq)]
    for q, p in planted.items():
        seqs[q] = planted_query(rng, oprofs[p], SIZES[p], flank=10)
    return profs, seqs


@pytest.fixture(scope="module")
def world(dcp, oracle64):
    return build_world(dcp, oracle64)


class CallerBuffer:
    def __init__(self, cap, words=6):
        self.cap = cap
        self.buf = torch.full((cap + GUARD, words), FILL_I32, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((1,), 77, dtype=torch.int32, device="cuda")  # a scan zeroes it first

    @property
    def count(self):
        return int(self.cnt.cpu()[0])

    def rows(self):
        return np.ascontiguousarray(self.buf.cpu().numpy()).view(np.uint32)

    def records(self, dtype, n):
        return self.rows()[:n].reshape(-1).view(dtype)

    def untouched_from(self, row):
        raw = self.rows()[row:]
        assert (raw == FILL).all(), np.argwhere(raw != FILL)[:4]


def fetch64(dcp, sc, room):
    out = np.zeros(room, dcp.HIT64_DTYPE)
    nh = C.c_uint(0)
    rc = sc._lib.dcp_gpu_fetch_hits64(sc._c, out.ctypes.data, room, C.byref(nh))
    return rc, nh.value, out


def check_caller_buffer(dcp, sc, rescan, want):
    """cap = n + 3, n and n - 1 (module docstring)"""
    n = len(want)
    assert n >= 4
    keys = [tuple(r) for r in words_of(want).tolist()]
    assert len(set(keys)) == n
    try:
        for cap in (n + 3, n, n - 1):
            cb = CallerBuffer(cap)
            sc.set_hit_buffer64(cb.buf.data_ptr(), cap, cb.cnt.data_ptr())
            rescan()
            assert sc.hit_buffer64() == (cb.buf.data_ptr(), cb.cnt.data_ptr(), cap)
            assert cb.count == n, (cap, cb.count, n)
            cb.untouched_from(min(cap, n))
            rc, nh, out = fetch64(dcp, sc, n + 8)
            assert nh == n
            if cap >= n:
                assert rc == 0 and same_bits(out[:n], want)
                assert same_bits(by_key(cb.records(dcp.HIT64_DTYPE, n)), want)
                assert same_bits(sc.hits(), want)
            else:
                assert rc == dcp.RC_ENOMEM
                held = [tuple(r) for r in words_of(cb.records(dcp.HIT64_DTYPE, cap)).tolist()]
                assert len(set(held)) == cap and set(held) <= set(keys)
                with pytest.raises(dcp.DcpError) as e:
                    sc.hits()
                assert e.value.rc == dcp.RC_ENOMEM
    finally:
        sc.set_hit_buffer64(None, 0, None)
    before = cb.rows().copy()
    rescan()
    assert same_bits(sc.hits(), want)
    hits_dev, _, own_cap = sc.hit_buffer64()
    assert hits_dev != cb.buf.data_ptr() and own_cap >= n
    assert np.array_equal(cb.rows(), before) and cb.count == n  # the caller's memory is the caller's again


@pytest.mark.parametrize("multi", [True, False], ids=["multi", "uni"])
@pytest.mark.parametrize("kernel", [0, 1, 4])
def test_caller_buffer(dcp, world, kernel, multi):
    """Kernels 0, 1 and 4, multi- and uni-hit, and a ranged scan into the caller's buffer."""
    profs, seqs = world
    ran = dcp.KERNEL_QLANE64 if kernel == 4 else dcp.KERNEL_ROWSWEEP
    sc = dcp.Scanner(0)
    try:
        sc.upload_db(profs)
        sc.upload_seqs(seqs)

        def rescan(q_range=None):
            sc.scan(multi, False, 10.0, keep_scores=False, kernel=kernel, q_range=q_range)
            assert sc.last_scan_kernel == ran

        rescan()
        want = sc.hits().copy()
        assert set(PLANTED.items()) <= set(zip(want["seq_idx"].tolist(), want["profile_idx"].tolist()))
        check_caller_buffer(dcp, sc, rescan, want)
        # a ranged scan: the range's slice of the list, the sequence indices those of the resident batch
        q0, q1 = 17, 59
        part = want[(want["seq_idx"] >= q0) & (want["seq_idx"] < q1)]
        assert 2 <= len(part) < len(want)
        cb = CallerBuffer(len(part))
        sc.set_hit_buffer64(cb.buf.data_ptr(), cb.cap, cb.cnt.data_ptr())
        rescan((q0, q1))
        assert cb.count == len(part)
        assert same_bits(by_key(cb.records(dcp.HIT64_DTYPE, len(part))), part) and same_bits(sc.hits(), part)
        cb.untouched_from(len(part))
    finally:
        sc.close()


def redo_world(dcp, oracle64):
    """Planted multi-copy queries (k = 1 .. 5 copies, back to back and spaced) of a 10-node and a 257-node profile among
    random queries and profiles: the pairs whose best path re-enters B leave kernel 4 through its redo lists."""
    rng = np.random.default_rng(4100)
    fams = [planted_family(oracle64, M) for M in (10, 257)]
    params = [fams[0][0], pfam_like_params(rng, 70), fams[1][0], pfam_like_params(rng, 130)]
    profs, _ = make_profiles(dcp, oracle64, params, [ENTRY_DIST_OCCUPANCY] * len(params))
    seqs = [s for _, _, s in fams[0][2]] + [s for k, _, s in fams[1][2] if k <= 2]
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(30, 201, 60)]
    order = rng.permutation(len(seqs))
    return profs, [seqs[i] for i in order]


def test_redo_pairs_and_the_repeated_scan_use_the_caller_buffer(dcp, oracle64):
    """Kernel 4's redo launches write into the caller's buffer; and when its redo lists overflow (test-hooks build, three
    pairs per list) dcp_gpu_sync repeats the scan with the row sweep, which zeroes the caller's counter first: the
    counter is n, not more, and no record appears twice."""
    profs, seqs = redo_world(dcp, oracle64)
    npairs = len(profs) * len(seqs)
    hk = dcp.Scanner(0, lib=dcp.load_testhooks())
    try:
        hk.upload_db(profs)
        hk.upload_seqs(seqs)
        hk.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
        want = hk.hits().copy()
        n = len(want)
        assert n >= 10
        cb = CallerBuffer(n + 3)
        hk.set_hit_buffer64(cb.buf.data_ptr(), cb.cap, cb.cnt.data_ptr())
        hk.scan(True, False, 10.0, keep_scores=False, kernel=dcp.KERNEL_QLANE64)
        assert hk.last_scan_kernel == dcp.KERNEL_QLANE64
        redo = hk.last_scan_redo_pairs
        assert 0 < redo < npairs, redo
        assert cb.count == n
        assert same_bits(by_key(cb.records(dcp.HIT64_DTYPE, n)), want) and same_bits(hk.hits(), want)
        cb.untouched_from(n)

        hk.test_set_redo_cap(3)
        cb = CallerBuffer(n + 3)
        hk.set_hit_buffer64(cb.buf.data_ptr(), cb.cap, cb.cnt.data_ptr())
        hk.scan(True, False, 10.0, keep_scores=False, kernel=dcp.KERNEL_QLANE64)  # sync: the lists are looked at
        assert hk.last_scan_kernel == dcp.KERNEL_ROWSWEEP
        assert cb.count == n, (cb.count, n)
        held = cb.records(dcp.HIT64_DTYPE, n)
        assert len(set(zip(held["seq_idx"].tolist(), held["profile_idx"].tolist()))) == n
        assert same_bits(by_key(held), want) and same_bits(hk.hits(), want)
        cb.untouched_from(n)
        hk.test_set_redo_cap(0)
        hk.set_hit_buffer64(None, 0, None)
    finally:
        hk.close()


def raw_hit_buffer(sc, name):
    h, nh, cap = C.c_void_p(), C.c_void_p(), C.c_uint(0)
    rc = getattr(sc._lib, name)(sc._c, C.byref(h), C.byref(nh), C.byref(cap))
    return rc, h.value, nh.value, cap.value


def test_refusals_and_independent_registrations(dcp, world):
    """dcp_gpu_hit_buffer64 answers double scans only, dcp_gpu_hit_buffer float scans only; the float and the double
    registration are two: a scan writes to the one of its DB's precision and leaves the other's memory alone."""
    profs, seqs = world
    fprofs = [dcp.ProteinProfile.sample(7 + i, M) for i, M in enumerate((30, 90))]
    sc = dcp.Scanner(0)
    try:
        rc, *_ = raw_hit_buffer(sc, "dcp_gpu_hit_buffer64")
        assert rc == dcp.RC_EINVAL and "no scan yet" in sc._lib.dcp_gpu_last_error(sc._c).decode()
        with pytest.raises(dcp.DcpError) as e:
            sc.hit_buffer64()
        assert e.value.rc == dcp.RC_EINVAL
        # pointer and counter come together, and a buffer has room
        one = torch.zeros(6, dtype=torch.int32, device="cuda")
        for args in ((one.data_ptr(), 1, None), (None, 1, one.data_ptr()), (one.data_ptr(), 0, one.data_ptr())):
            with pytest.raises(dcp.DcpError) as e:
                sc.set_hit_buffer64(*args)
            assert e.value.rc == dcp.RC_EINVAL and "together" in str(e.value)
        assert sc._lib.dcp_gpu_set_hit_buffer64(None, None, 0, None) == dcp.RC_EINVAL
        assert sc._lib.dcp_gpu_hit_buffer64(sc._c, None, None, None) == dcp.RC_EINVAL

        f32, f64 = CallerBuffer(256, words=4), CallerBuffer(64)
        sc.set_hit_buffer(f32.buf.data_ptr(), f32.cap, f32.cnt.data_ptr())
        sc.set_hit_buffer64(f64.buf.data_ptr(), f64.cap, f64.cnt.data_ptr())
        sc.upload_db(fprofs)
        sc.upload_seqs(seqs)
        sc.scan(True, False, -1e30, keep_scores=False)  # a float scan: every finite LRT is a hit
        nf = f32.count
        assert 0 < nf <= f32.cap and same_float_records(dcp, f32.records(dcp.HIT_DTYPE, nf), sc.hits())
        f32.untouched_from(nf)
        f64.untouched_from(0)
        assert f64.count == 77
        rc, *_ = raw_hit_buffer(sc, "dcp_gpu_hit_buffer64")
        assert rc == dcp.RC_EINVAL and "float DB" in sc._lib.dcp_gpu_last_error(sc._c).decode()
        rc, h, nh, cap = raw_hit_buffer(sc, "dcp_gpu_hit_buffer")
        assert (rc, h, nh, cap) == (0, f32.buf.data_ptr(), f32.cnt.data_ptr(), f32.cap)

        float_rows = f32.rows().copy()
        sc.upload_db(profs)
        sc.scan(True, False, 10.0, keep_scores=False, kernel=dcp.KERNEL_QLANE64)
        nd = f64.count
        assert 4 <= nd <= f64.cap and same_bits(by_key(f64.records(dcp.HIT64_DTYPE, nd)), sc.hits())
        f64.untouched_from(nd)
        assert np.array_equal(f32.rows(), float_rows) and f32.count == nf
        assert sc.hit_buffer64() == (f64.buf.data_ptr(), f64.cnt.data_ptr(), f64.cap)
        rc, *_ = raw_hit_buffer(sc, "dcp_gpu_hit_buffer")
        assert rc == dcp.RC_EINVAL and "dcp_hit64" in sc._lib.dcp_gpu_last_error(sc._c).decode()
        # taking the double registration back leaves the float one in force
        sc.set_hit_buffer64(None, 0, None)
        sc.upload_db(fprofs)
        sc.scan(True, False, -1e30, keep_scores=False)
        rc, h, nh, cap = raw_hit_buffer(sc, "dcp_gpu_hit_buffer")
        assert (rc, h, nh, cap) == (0, f32.buf.data_ptr(), f32.cnt.data_ptr(), f32.cap) and f32.count == nf
    finally:
        sc.close()


def same_float_records(dcp, got, want):
    got = got[np.lexsort((got["profile_idx"], got["seq_idx"]))]
    return len(got) == len(want) and np.array_equal(np.ascontiguousarray(got).view(np.uint32),
                                                    np.ascontiguousarray(want).view(np.uint32))
