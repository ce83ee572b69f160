"""The two-stage query-lane kernel (viterbi_qlane2_kernel) on a short last tile (runs on a real MI355X).

A profile's last tile is padded to 8 nodes; the kernel sweeps a last tile behind the first with only NV = 2, 4, 6 or 8
of them, the v = core_size - 8 (T - 1) real ones rounded up to a pair (dcp_qlane.hip, QL2_SWEEP_LAST).  A variant that
runs one node too few loses a real match state; one whose group-1 gathers or waits are wrong reads another row.  Both
change bits:

  profiles   sampled, M = 9 .. 24: T = 2 and T = 3 tiles, so each of the 8 remainders puts its last tile once on
             stage 1 and once on stage 0 -- all eight (stage, NV) variants; M = 8, whose only tile is `first && last`
             and stays at NV = 8; M = 30 and 33 (the benchmark's smallest shapes, T = 4 and 5)
  queries    per profile one query carrying the most likely codon of each match state (as bench.py's plant_hits builds
             it) between 10 random bases on either side: the best path runs through the LAST real node and E is
             decided there; random queries of 1 .. 6 nt and of 60 .. 120 nt
  batches    3, 65 and 257 queries: a partial group, a second group in the block, a second block
  modes      multi-hit and uni-hit on the default DB, multi-hit on a one-layout DB.  The consensus queries re-enter the
             core in multi-hit, so those pairs go through the redo lists: the scores compared are the union of what
             the query-lane kernel published and what the row sweep re-scored

`null` and `alt` of EVERY pair equal the oracle's float32 recursion fed the device's own tables, as uint32.
"""
import numpy as np
import pytest
import torch  # noqa: F401  before the product's library: both bring a HIP runtime, and torch must see the device too

import test_gpu_parity as tp
from oracle_py import ENTRY_DIST_OCCUPANCY

pytestmark = pytest.mark.gpu

CORE_SIZES = (8,) + tuple(range(9, 25)) + (30, 33)
BATCHES = (3, 65, 257)
CASES = [(True, False), (False, False), (True, True)]  # (multi, one_layout)
KT = 8


def variant_of(M):
    """(stage that sweeps the last tile, nodes it runs there): the kernel's dispatch restated from core_size."""
    T = -(-M // KT)
    if T == 1:
        return (0, KT)  # first && last
    v = M - (T - 1) * KT
    return ((T - 1) & 1, (v + 1) & ~1)


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


def consensus_query(rng, prof, flank=10):
    """The most likely codon of every match state (bench.py, plant_hits) between `flank` random bases."""
    codon = prof.match_dist[:, 4:].reshape(-1, 5, 5, 5)[:, :4, :4, :4].reshape(-1, 64).argmax(axis=1)
    core = np.stack([(codon >> 4) & 3, (codon >> 2) & 3, codon & 3], axis=1).reshape(-1).astype(np.uint8)
    assert len(core) == 3 * prof.core_size
    return np.concatenate([rng.integers(0, 4, flank, dtype=np.uint8), core, rng.integers(0, 4, flank, dtype=np.uint8)])


_shared = {}


def shared(dcp):
    if not _shared:
        rng = np.random.default_rng(9200)
        profiles = tp.make_profiles(dcp, [(9200 + M, M, ENTRY_DIST_OCCUPANCY, 0.01) for M in CORE_SIZES])
        cons = {p.core_size: consensus_query(rng, p) for p in profiles}
        short = [rng.integers(0, 4, L, dtype=np.uint8) for L in range(1, 7)]
        longer = [rng.integers(0, 4, L, dtype=np.uint8) for L in (60, 61, 75, 88, 97, 104, 119, 120)]
        # the batch of 3 is the first three: a last tile of 3 nodes on stage 1, one of 5 nodes on stage 0, a short query
        head = [cons.pop(11), cons.pop(21), short.pop(2)]
        _shared["profiles"] = profiles
        _shared["queries"] = head + list(cons.values()) + short + longer
        _shared["oracle"] = {}
    return _shared["profiles"], _shared["queries"], _shared["oracle"]


def test_profiles_reach_every_variant(dcp):
    profiles, queries, _ = shared(dcp)
    behind_first = {variant_of(p.core_size) for p in profiles if p.core_size > KT}
    assert behind_first == {(s, nv) for s in (0, 1) for nv in (2, 4, 6, 8)}
    assert variant_of(8) == (0, 8) and variant_of(30) == (1, 6) and variant_of(33) == (0, 2)
    assert len(queries) == len(CORE_SIZES) + 6 + 8 and max(len(q) for q in queries) <= 120


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("multi,one_layout", CASES, ids=lambda v: None)
def test_short_last_tile_on_both_stages(dcp, oracle32, scanner, multi, one_layout, nq):
    profiles, queries, cache = shared(dcp)
    src = np.arange(nq) % len(queries)
    seqs = [queries[i] for i in src]
    scanner.upload_db(profiles, expand_on_host=False, one_layout=one_layout)
    assert scanner.one_layout == one_layout
    if (multi, one_layout) not in cache:  # the oracle scores the distinct queries once per mode, on the device's tables
        cache[(multi, one_layout)] = tp.oracle_dp_on_product_tables(dcp, oracle32, scanner, profiles, queries, multi, False, False)
    on, oa = (x[src] for x in cache[(multi, one_layout)])
    scanner.upload_seqs(seqs)
    scanner.scan(multi, False, 1e30, keep_scores=True, kernel=dcp.KERNEL_QLANE2)
    assert scanner.last_scan_kernel == dcp.KERNEL_QLANE2
    gn, ga = scanner.scores()
    redo = scanner.last_scan_redo_pairs
    u32 = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    bad = np.argwhere((u32(gn) != u32(on)) | (u32(ga) != u32(oa)))
    if len(bad):
        q, p = int(bad[0][0]), int(bad[0][1])
        raise AssertionError("%d of %d pairs differ (%d redo pairs); first: query %d (distinct query %d, %d nt) x profile of %d "
                             "nodes (stage, NV) = %r: device null %r alt %r, oracle %r %r" % (
                                 len(bad), gn.size, redo, q, src[q], len(seqs[q]), profiles[p].core_size,
                                 variant_of(profiles[p].core_size), gn[q, p], ga[q, p], on[q, p], oa[q, p]))
    # feedback pairs: a consensus query re-enters its own profile's core in multi-hit; uni-hit has no E -> B edge
    assert redo > 0 if multi else redo == 0, redo
