"""forward_pairs, posterior_pairs and mea_pairs taking turns on one context, each with another list: whatever one kind
of call sized or filled -- the special transitions, the two lists, the offsets, the scores, the row records, the wide
sweep's work area and its stride, the profile table -- must not show in the next call of another kind.  Every result is
held in bits to the same call on a fresh context with the same DB and batch, and every call moves its own clock only.
The clocks are compared exactly: each is a value stored at the end of its call, not formed from events at every look.

Six sampled profiles of 2, 64, 65, 129, 257 and 513 nodes: 1, 1, 2 and 4 nodes per lane in registers, then the wide
sweep at two and at three chunks, so that the work area's stride shrinks and grows between calls.  Queries of 1, 5, 6, 37
and 100 nt."""
import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits
from test_forward_pairs import PRECISIONS

SIZES = (2, 64, 65, 129, 257, 513)
LENGTHS = (1, 5, 6, 37, 100)
# (sequence, profile) lists, by position in LENGTHS and SIZES
WIDE_AND_TINY = (np.array([4, 0, 2]), np.array([5, 0, 5]))  # the 513 profile and the 2 profile
NARROWER = (np.array([4, 1, 3, 0]), np.array([4, 0, 4, 0]))  # only 257 and 2: a smaller stride in the same work area
EVERY_CLASS = (np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 4, 3, 4]),
               np.array([0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 3, 5]))  # (4, 5) twice
EMPTY = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
REORDER = (3, 5, 0, 4, 2, 1)
KINDS = ("forward", "posterior", "mea")


def call(sc, kind, lst):
    return getattr(sc, kind + "_pairs")(*lst)


def same(kind, got, want):
    if kind == "forward":  # null, alt
        return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
    if kind == "posterior":  # row_off, begin, end, core, alt_fwd, alt_bwd
        return np.array_equal(got[0], want[0]) and all(np.array_equal(bits(g), bits(w)) for g, w in zip(got[1:], want[1:]))
    paths, posts, gain, fwd = got
    return (len(paths) == len(want[0]) and all(g.tobytes() == w.tobytes() for g, w in zip(paths, want[0])) and
            all(np.array_equal(bits(g), bits(w)) for g, w in zip(posts, want[1])) and
            np.array_equal(bits(gain), bits(want[2])) and np.array_equal(bits(fwd), bits(want[3])))


def clocks(sc):
    return {"forward": sc.forward_kernel_ms, "posterior": sc.posterior_kernel_ms, "mea": sc.mea_kernel_ms}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_calls_of_three_kinds_share_one_context(dcp, precision):
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
    profs = [dcp.ProteinProfile.sample(4100 + i, M, cfg, f"S{i}", precision=precision) for i, M in enumerate(SIZES)]
    rng = np.random.default_rng(4200 + precision)
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in LENGTHS]

    def fresh(kind, lst, db=profs):
        sc = dcp.Scanner(0)
        sc.upload_db(db)
        sc.upload_seqs(seqs)
        out = call(sc, kind, lst)
        sc.close()
        return out

    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    assert all(v < 0 for v in clocks(sc).values())

    def step(kind, lst, want, label):
        before = clocks(sc)
        got = call(sc, kind, lst)
        after = clocks(sc)
        assert same(kind, got, want), label
        assert after[kind] > 0.0, label
        assert all(after[k] == before[k] for k in KINDS if k != kind), (label, before, after)

    mea_wide = fresh("mea", WIDE_AND_TINY)
    post_every = fresh("posterior", EVERY_CLASS)
    step("mea", WIDE_AND_TINY, mea_wide, 1)
    step("forward", NARROWER, fresh("forward", NARROWER), 2)
    step("posterior", EVERY_CLASS, post_every, 3)
    before = clocks(sc)
    null, alt = sc.forward_pairs(*EMPTY)
    row_off, begin = sc.posterior_pairs(*EMPTY)[:2]
    paths, posts, gain, fwd = sc.mea_pairs(*EMPTY)
    assert len(null) == len(alt) == len(begin) == len(paths) == len(posts) == len(gain) == len(fwd) == 0
    assert row_off.tolist() == [0] and clocks(sc) == before  # 4: an empty list moves no clock
    sc.test_set_mea_budget(1)  # every pair a round of its own
    step("mea", EVERY_CLASS, fresh("mea", EVERY_CLASS), 5)
    sc.test_set_mea_budget(0)
    step("posterior", EVERY_CLASS, post_every, 6)
    step("mea", WIDE_AND_TINY, mea_wide, 7)
    other = [profs[i] for i in REORDER]
    sc.upload_db(other)  # the same profiles in another order: the profile table goes with the DB
    step("forward", EVERY_CLASS, fresh("forward", EVERY_CLASS, other), 8)
    sc.close()
