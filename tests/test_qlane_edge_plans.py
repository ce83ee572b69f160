"""The batches of tests/test_qlane_edges.py (families B, C, D) and the plans dcp_plan_query_slots makes for them.

The query-lane kernels sweep a batch as the planner packs it: 64-query groups (one wavefront's lanes; a group runs for
`Lwave` = its longest member's rows), listed per wavefront slot, each at its `rowbase` of the slot's plane column.  Which
ring slot, which flag value, which park row a case reaches is decided by that plan, so every batch below is built for
one shape and the shape is ASSERTED here, on the CPU (dcp_plan_query_slots is host code) -- the GPU cases make the same
assertion before they scan.  A change to the planner that turns a case into a different one fails here first.
"""
import numpy as np

from test_query_slots import check_invariants, group_rows, plan

# ---- family B: the rows of one group -----------------------------------------------------------------------------
# Lwave < kRingSkew = 4 (1, 2, 3), every Lwave mod 5 below and above the five-row unrolling, the 16-row ring's wraps
# (15, 16, 17, 31, 32, 33), and longer ones at both sides of a multiple of 16 and of 5
B_LWAVES = list(range(1, 46)) + [79, 80, 81, 159, 160, 161]
B_CORE_SIZES = (5, 12, 20, 29)  # T = 1, 2, 3, 4 tiles of 8 nodes


def b_lens(Lwave, n, mixed):
    """n = 64 or 128 query lengths in caller order: all Lwave, or (mixed) lane i of length 1 + i % Lwave with the
    longest last -- lanes of 1 nt next to the group's Lwave."""
    if not mixed:
        return np.full(n, Lwave, np.uint32)
    return np.array([1 + i % Lwave for i in range(n - 1)] + [Lwave], np.uint32)


def b_expected_groups(Lwave, n, mixed):
    """(first, n, rowbase, lmax) per group in slot order: one group per slot, the longer first."""
    lens = np.sort(b_lens(Lwave, n, mixed))
    if n == 64:
        return [(0, 64, 0, Lwave)]
    return [(64, 64, 0, Lwave), (0, 64, 0, int(lens[63]))]


# ---- family C: groups sharing a slot -----------------------------------------------------------------------------
# name -> lengths of the 64-query groups in caller order (queries of a group have one length).  The shapes were found
# by running the planner over candidates; they are pinned in C_SHAPES as [(rowbase, Lwave), ...] per slot.
C_BATCHES = {
    # 24 groups: the long one alone in its slot next to slots of 8, 8 and 7 short groups whose rowbases step by 14:
    # 0, 14, 28, ... 98 = every even residue mod 16
    "long_alone": [100] + [3] * 23,
    # 9 groups: groups of Lwave 1, 2, 3 swept BEHIND a long group of their slot (rowbase 40 .. 62)
    "short_behind_long": [60, 50, 40, 30, 3, 2, 1, 1, 1],
    # 17 groups: one to six groups per slot, Lwave 1 .. 31 at rowbases of every even residue mod 16 but one (the
    # three batches together reach all eight, asserted below)
    "one_to_six": [200, 31, 30, 17, 16, 15, 3, 2, 1, 1, 2, 3, 5, 7, 9, 11, 13],
}
C_SHAPES = {
    "long_alone": [[(14 * i, 3) for i in range(8)], [(14 * i, 3) for i in range(8)], [(0, 100)],
                   [(14 * i, 3) for i in range(7)]],
    "short_behind_long": [[(0, 40), (50, 2), (62, 1)], [(0, 50), (60, 1)], [(0, 60)], [(0, 30), (40, 3), (54, 1)]],
    "one_to_six": [[(0, 200)], [(0, 17), (28, 16), (54, 11), (76, 5), (92, 2), (104, 1)],
                   [(0, 31), (42, 13), (66, 9), (86, 3), (100, 1)], [(0, 30), (40, 15), (66, 7), (84, 3), (98, 2)]],
}
# a ranged scan re-plans for its own queries: groups 1 .. 8 of "one_to_six" (caller indices 64 .. 576)
C_RANGE = ("one_to_six", 64, 576)
C_RANGE_SHAPE = [[(0, 31), (42, 1)], [(0, 30), (40, 2)], [(0, 16), (26, 15)], [(0, 17), (28, 3)]]
C_CORE_SIZES = (5, 12, 20, 29, 100)  # T = 1, 2, 3, 4, 13


def c_lens(name):
    return np.repeat(np.array(C_BATCHES[name], np.uint32), 64)


def slot_shape(p):
    """[[(rowbase, lmax), ...] per slot] of a plan."""
    sf = p["slot_first"]
    return [[(int(g[2]), int(g[3])) for g in p["groups"][sf[s]:sf[s + 1]]] for s in range(p["nb"] * p["slots"])]


# ---- family D: fill ----------------------------------------------------------------------------------------------
D_NQ = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)
D_POOL = 1 + (np.arange(513, dtype=np.uint32) * 37) % 60  # lengths 1 .. 60 in caller order; a batch is a prefix


def d_lens(nq):
    return D_POOL[:nq].copy()


# nq -> (blocks, groups, queries of the partial group (0: none), slots without a group) with four slots per block
D_SHAPES = {1: (1, 1, 1, 3), 2: (1, 1, 2, 3), 63: (1, 1, 63, 3), 64: (1, 1, 0, 3), 65: (1, 2, 1, 2), 127: (1, 2, 63, 2),
            128: (1, 2, 0, 2), 129: (1, 3, 1, 1), 191: (1, 3, 63, 1), 192: (1, 3, 0, 1), 193: (1, 4, 1, 0),
            255: (1, 4, 63, 0), 256: (1, 4, 0, 0), 257: (1, 5, 1, 0), 511: (1, 8, 63, 0), 512: (1, 8, 0, 0),
            513: (1, 9, 1, 0)}


def d_shape(p):
    sf = p["slot_first"]
    partial = [int(g[1]) for g in p["groups"] if g[1] != 64]
    assert len(partial) <= 1
    return (p["nb"], len(p["groups"]), partial[0] if partial else 0, int((np.diff(sf.astype(np.int64)) == 0).sum()))


def assert_b_plan(dcp, Lwave, n, mixed, slots):
    lens = b_lens(Lwave, n, mixed)
    p = plan(dcp, lens, slots)
    check_invariants(p)
    want = b_expected_groups(Lwave, n, mixed)
    assert p["nb"] == (1 if slots == 4 else len(want)), (Lwave, n, mixed, p["nb"])
    assert [tuple(int(x) for x in g) for g in p["groups"]] == want, (Lwave, n, mixed, p["groups"])
    assert p["plane_rows"] == group_rows(Lwave)
    if mixed and Lwave > 1:
        assert lens.min() == 1  # a lane of one row in a group of Lwave rows
    return p


def assert_c_plan(dcp, lens, shape):
    p = plan(dcp, lens, 4)
    check_invariants(p)
    assert p["nb"] == 1 and slot_shape(p) == shape, slot_shape(p)
    return p


def assert_d_plan(dcp, nq):
    p = plan(dcp, d_lens(nq), 4)
    check_invariants(p)
    assert d_shape(p) == D_SHAPES[nq], (nq, d_shape(p))
    if nq % 64:  # the partial group holds the SHORTEST queries
        part = [g for g in p["groups"] if g[1] != 64][0]
        assert part[0] == 0 and part[3] == np.sort(d_lens(nq))[nq % 64 - 1]
    if nq <= 64:  # what KERNEL_QLANE runs such a batch with: one slot per block, one group
        p1 = plan(dcp, d_lens(nq), 1)
        check_invariants(p1)
        assert p1["nb"] == 1 and len(p1["groups"]) == 1
    return p


def test_family_b_plans(dcp):
    """Lwave = 1, 2, 3 (< kRingSkew), Lwave mod 5 = 0 .. 4, the ring's wraps: one group per slot at rowbase 0 whose
    Lwave is the case's, for batches of 64 (four- and one-slot blocks) and 128 queries, uniform and mixed."""
    for Lwave in B_LWAVES:
        for mixed in (False, True):
            assert_b_plan(dcp, Lwave, 64, mixed, 4)
            assert_b_plan(dcp, Lwave, 64, mixed, 1)
            assert_b_plan(dcp, Lwave, 128, mixed, 4)
    assert {L % 5 for L in B_LWAVES if L < 5} | {0} == set(range(5)) and {L % 16 for L in B_LWAVES} == set(range(16))


def test_family_c_plans(dcp):
    """rowbase != 0: the pinned shapes, one to six (and eight) groups per slot, every even rowbase residue mod 16,
    groups of Lwave <= 3 behind a long group, a long group alone in its slot; the ranged scan's own plan."""
    residues, per_slot = set(), set()
    for name in C_BATCHES:
        p = assert_c_plan(dcp, c_lens(name), C_SHAPES[name])
        residues |= {int(g[2]) % 16 for g in p["groups"]}
        per_slot |= {len(s) for s in C_SHAPES[name]}
    assert residues == {0, 2, 4, 6, 8, 10, 12, 14}
    assert {int(g[2]) % 16 for g in plan(dcp, c_lens("long_alone"), 4)["groups"]} == residues  # one batch has them all
    assert per_slot >= {1, 2, 3, 5, 6, 7, 8}
    assert [(0, 100)] in C_SHAPES["long_alone"] and [(0, 200)] in C_SHAPES["one_to_six"]
    behind = [(rb, L) for s in C_SHAPES["short_behind_long"] for rb, L in s if L <= 3]
    assert len(behind) == 5 and all(rb >= 40 for rb, _ in behind) and {L for _, L in behind} == {1, 2, 3}
    name, q0, q1 = C_RANGE
    assert_c_plan(dcp, c_lens(name)[q0:q1], C_RANGE_SHAPE)


def test_family_d_plans(dcp):
    """nq = 1 .. 513: lanes without a query (the partial group is the shortest queries'), slots without a group
    (g0 == g1); batches of mixed lengths up to 513 queries pack into one block of two or three groups per slot."""
    for nq in D_NQ:
        assert_d_plan(dcp, nq)
    assert D_POOL.min() == 1 and D_POOL.max() == 60


# ---- family E: more tasks than resident blocks --------------------------------------------------------------------
def e_lens(nq):
    """64 queries of 1 .. 40 nt (one group: one task per profile), or 300 of 24 nt (five groups of one length: two
    blocks, the second with three empty slots -- two tasks per profile)."""
    return (1 + (np.arange(nq, dtype=np.uint32) * 7) % 40) if nq <= 64 else np.full(nq, 24, np.uint32)


def assert_e_plan(dcp, nq, slots):
    p = plan(dcp, e_lens(nq), slots)
    check_invariants(p)
    assert p["nb"] == (1 if nq <= 64 else 2), p["nb"]
    if nq > 64:
        assert slot_shape(p) == [[(0, 24)]] * 5 + [[]] * 3, slot_shape(p)
    return p


def test_family_e_plans(dcp):
    assert_e_plan(dcp, 64, 1)
    assert_e_plan(dcp, 64, 4)
    assert_e_plan(dcp, 300, 4)
