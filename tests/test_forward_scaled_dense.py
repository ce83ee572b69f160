"""The dense Forward scan by the scaled sweeps (runs on a real MI355X): dcp_gpu_forward_dense_scaled /
Scanner.forward_dense_scaled (csrc/dcp_gpu.hip, csrc/dcp_forward_scaled.hip).

Nothing here has a tolerance of its own.  A pair's sweep does not depend on what else is in a launch, so every entry of
the dense matrices is compared IN BITS with forward_pairs_scaled of the full q-major list -- whether those are right is
tests/test_forward_scaled.py's business.  The fit on the result is compared with the host twin on the fetched matrices,
as tests/test_forward_dense.py compares forward_dense's.  The world is that file's: profiles on every class edge,
sequences of 1 .. 40 nt, rounds that cut the line of pairs inside classes and between them."""
import numpy as np
import pytest

import test_forward_chain_premises as pr
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, refused
from test_forward_dense import compare_exp_fits, dense_world, full_list, host_exp_fits, same_matrices
from test_forward_pairs import FLAGS, NEG_INF, PRECISIONS


def scaled_pairs_as_matrices(sc, multi=True, h3=False):
    sq, pr_ = full_list(sc)
    nl, al = sc.forward_pairs_scaled(sq, pr_, multi, h3)
    return nl.reshape(sc.nseqs, sc.nprofiles), al.reshape(sc.nseqs, sc.nprofiles)


def dense_scaled(sc, multi=True, h3=False):
    sc.forward_dense_scaled(multi, h3)
    return sc.forward_scores()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dense_scaled_equals_the_scaled_pair_list(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    sc = dcp.Scanner(0)
    refused(dcp, sc, sc.forward_dense_scaled)  # no DB
    sc.upload_db(profs + [eps0])
    refused(dcp, sc, sc.forward_dense_scaled)  # no batch
    sc.upload_seqs(seqs)
    refused(dcp, sc, sc.forward_scores)  # none computed yet
    assert sc.forward_dense_kernel_ms() < 0 and not sc.forward_dense_is_scaled
    seen = set()
    for multi, h3 in FLAGS:
        got = dense_scaled(sc, multi, h3)
        assert sc.forward_dense_kernel_ms() > 0 and sc.forward_dense_is_scaled and sc.last_forward_scaled_redo_pairs == 0
        want = scaled_pairs_as_matrices(sc, multi, h3)
        assert got[0].shape == (len(seqs), len(profs) + 1) and same_matrices(got, want), (precision, multi, h3)
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
        for q, s in enumerate(seqs):  # the epsilon-0 profile: -inf twice where L mod 3 != 0
            if len(s) % 3:
                assert got[0][q, -1] == NEG_INF and got[1][q, -1] == NEG_INF
        assert np.isfinite(got[1][:, :-1]).sum() > got[1][:, :-1].size // 2
        seen.add(got[1].tobytes())
        # the fit runs on the result unchanged: the host twin's bits on the fetched matrices
        for k in (2, len(seqs)):
            compare_exp_fits(sc.fit_exp_tail(k, "forward"), host_exp_fits(dcp, got[0], got[1], k), (precision, multi, h3, k))
    assert len(seen) == len(FLAGS)  # the flags reach the sweeps
    # forward_dense_is_scaled follows the last call; the log-space scan's matrices differ in bits somewhere
    sc.forward_dense()
    assert not sc.forward_dense_is_scaled
    log_space = sc.forward_scores()
    sc.forward_dense_scaled()
    assert sc.forward_dense_is_scaled and not same_matrices(sc.forward_scores(), log_space)
    # void after an upload
    sc.upload_seqs(seqs)
    refused(dcp, sc, sc.forward_scores)
    refused(dcp, sc, lambda: sc.fit_exp_tail(2))
    assert not sc.forward_dense_is_scaled
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounds_caps_and_bands_change_no_bit(dcp, precision):
    profs, eps0, seqs = dense_world(dcp, precision)
    P, B = len(profs), len(seqs)
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    base = dense_scaled(sc)
    assert same_matrices(base, scaled_pairs_as_matrices(sc))
    for npairs in (1, 7, P - 1, P + 1):
        sc.test_set_dense_round(npairs)
        assert same_matrices(dense_scaled(sc), base), (precision, npairs)
    sc.test_set_dense_round(0)
    for cap in (1, 3):
        sc.test_set_forward_waves(cap)
        assert same_matrices(dense_scaled(sc), base), (precision, cap)
    sc.test_set_dense_round(7)  # both at once, and a small band
    sc.test_set_forward_scale_band(4)
    assert same_matrices(dense_scaled(sc), base)
    sc.test_set_forward_waves(0)
    sc.test_set_dense_round(0)
    sc.test_set_forward_scale_band(0)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_redo_pairs_across_rounds(dcp, precision):
    """an out-of-range positive chain of 2 000 nodes and a wide delete-heavy profile among the world's: its column has
    forward_dense's bits, the others forward_pairs_scaled's, whatever the rounds"""
    profs, eps0, seqs = dense_world(dcp, precision)
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, pr.EPS)
    big = dcp.ProteinProfile.from_params(*pr.chain_params("positive", 2000), cfg, "POS2000", precision=precision)
    wide = dcp.ProteinProfile.from_params(*pr.chain_params("delete", 1100), cfg, "DEL1100", precision=precision)
    mine = profs[:3] + [big] + profs[3:] + [wide]
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(mine)
    sc.upload_seqs(seqs)
    sc.forward_dense()
    log_space = sc.forward_scores()
    base = dense_scaled(sc)
    assert sc.last_forward_scaled_redo_pairs == len(seqs)
    assert same_matrices(base, scaled_pairs_as_matrices(sc))
    assert np.isfinite(base[1][:, 3]).all()
    assert np.array_equal(bits(base[0][:, 3]), bits(log_space[0][:, 3])) and np.array_equal(bits(base[1][:, 3]), bits(log_space[1][:, 3]))
    for npairs, cap in ((1, 0), (3, 1), (len(mine) + 1, 3)):
        sc.test_set_dense_round(npairs)
        sc.test_set_forward_waves(cap)
        assert same_matrices(dense_scaled(sc), base), (precision, npairs, cap)
        assert sc.last_forward_scaled_redo_pairs == len(seqs)
    sc.close()
