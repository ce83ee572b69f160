"""dcp_profile_from_parts64 (CPU): a double profile rebuilt from its stored double parts -- what unpacking a profile of
a double .dcp needs -- is the profile dcp_profile_new64 / dcp_profile_sample64 built, double and float parts in bits."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("entry", [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY])
@pytest.mark.parametrize("M", [2, 63, 64, 65, 512, 4096])
def test_round_trip_in_bits(dcp, entry, M):
    cfg = dcp.ProteinCfg(entry, 0.1)  # 0.1 is not a float value
    assert cfg.epsilon64 != cfg.epsilon
    p = dcp.ProteinProfile.sample(7 + M, M, cfg, "PF00001.1", precision=64)
    q = dcp.ProteinProfile.from_parts64(*p.parts64(), cfg=cfg, accession=p.accession, consensus=p.consensus)
    assert q.precision == 64 and q.core_size == M and q.accession == p.accession and q.consensus == p.consensus
    assert bits(np.float64(q.epsilon64)) == bits(np.float64(0.1))
    for a, b in zip(p.parts64(), q.parts64()):
        assert np.array_equal(bits(a), bits(b))
    # the float parts: the double values rounded once, as dcp_profile_new64 leaves them
    for name in ("trans8", "null_dist", "insert_dist", "match_dist"):
        a, b = getattr(p, name), getattr(q, name)
        assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(bits(q.trans8), bits(q.parts64()[0].astype(np.float32)))


def test_refusals(dcp):
    p = dcp.ProteinProfile.sample(1, 5, precision=64)
    t8, nd, idist, md = p.parts64()

    def rc_of(f):
        with pytest.raises(dcp.DcpError) as e:
            f()
        return e.value.rc

    for i, part in enumerate((t8, nd, idist, md)):
        parts = [t8.copy(), nd.copy(), idist.copy(), md.copy()]
        parts[i].flat[parts[i].size - 1] = np.nan
        assert rc_of(lambda: dcp.ProteinProfile.from_parts64(*parts)) == dcp.RC_EINVAL
    rc = C.c_int(0)
    lib = dcp.lib
    args = (t8.ctypes.data, nd.ctypes.data, idist.ctypes.data, md.ctypes.data)
    for M, eps in ((0, 0.01), (4097, 0.01), (5, -0.5), (5, 1.5), (5, float("nan"))):
        assert not lib.dcp_profile_from_parts64(b"x", M, 2, eps, None, *args, C.byref(rc))
        assert rc.value == dcp.RC_EINVAL
    assert not lib.dcp_profile_from_parts64(b"x", 5, 2, 0.01, None, None, *args[1:], C.byref(rc))
    assert rc.value == dcp.RC_EINVAL
    # -inf is a value (MD / DD of the last node); a float profile has no double parts to give
    assert np.isneginf(t8).any()
    assert rc_of(lambda: dcp.ProteinProfile.sample(1, 5).parts64()) == dcp.RC_EINVAL
