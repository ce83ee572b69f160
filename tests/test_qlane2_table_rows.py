"""The two-stage query-lane kernel (viterbi_qlane2_kernel) at the ends of its LDS tables (runs on a real MI355X).

Both stages reach ONE insert / background table of 16-byte rows, and stage 1 its tile image, through DS immediates
formed from a riding base (dcp_qlane.hip, the layout above kL2TabIN): a wrong immediate reads another row -- of the
table, of an image, of the ring's flags -- and changes bits.  test_qlane_edges.py has the tiles, rows, ring and slots;
here every row of every table is read on both stages:

  profiles   sampled, M = 8, 9, 16, 17, 25 nodes: T = 1, 2, 2, 3, 4 tiles, so the last tile lands on stage 0 and on
             stage 1 and the one-tile profile takes the `first && last` sweep; a sampled profile's insert and
             background rows all differ
  queries    one order-5 de Bruijn sequence over ACGT (1 028 nt: each of the 1 024 five-base windows once, hence
             every row of the five word-length tables), poly-A and poly-T of 40 nt (codes 0 and 1023 row after row:
             first and last row of each table), random queries of 1 .. 6 nt (windows shorter than five bases)
  batches    3, 65 and 257 queries: a partial group, a second group in the block, a second block
  modes      multi-hit and uni-hit on the default DB, multi-hit on a one-layout DB

`null` and `alt` of EVERY pair equal the oracle's float32 recursion fed the device's own tables, as uint32.
"""
import numpy as np
import pytest
import torch  # noqa: F401  before the product's library: both bring a HIP runtime, and torch must see the device too

import test_gpu_parity as tp
from oracle_py import ENTRY_DIST_OCCUPANCY

pytestmark = pytest.mark.gpu

CORE_SIZES = (8, 9, 16, 17, 25)
BATCHES = (3, 65, 257)
CASES = [(True, False), (False, False), (True, True)]  # (multi, one_layout)


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


def de_bruijn(k, n):
    """The lexicographically least de Bruijn sequence B(k, n), opened: its first n - 1 symbols follow its last."""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return np.array(out + out[:n - 1], np.uint8)


def distinct_queries():
    rng = np.random.default_rng(9100)
    seq = de_bruijn(4, 5)
    assert len(seq) == 1028
    codes = sum(seq[i:i + 1024].astype(np.int64) << (2 * (4 - i)) for i in range(5))
    assert np.array_equal(np.sort(codes), np.arange(1024))  # every five-base window once
    return [seq, np.zeros(40, np.uint8), np.full(40, 3, np.uint8)] + [rng.integers(0, 4, L, dtype=np.uint8) for L in range(1, 7)]


_shared = {}


def shared(dcp):
    if not _shared:
        _shared["profiles"] = tp.make_profiles(dcp, [(9100 + M, M, ENTRY_DIST_OCCUPANCY, 0.01) for M in CORE_SIZES])
        _shared["queries"] = distinct_queries()
        _shared["oracle"] = {}
    return _shared["profiles"], _shared["queries"], _shared["oracle"]


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("multi,one_layout", CASES, ids=lambda v: None)
def test_every_table_row_on_both_stages(dcp, oracle32, scanner, multi, one_layout, nq):
    profiles, queries, cache = shared(dcp)
    assert [-(-p.core_size // 8) for p in profiles] == [1, 2, 2, 3, 4]  # tiles: last tile on stage 0, 1, 1, 0, 1
    # the de Bruijn sequence and the two homopolymers come first: the batch of 3 is these
    src = np.arange(nq) % len(queries)
    seqs = [queries[i] for i in src]
    scanner.upload_db(profiles, expand_on_host=False, one_layout=one_layout)
    assert scanner.one_layout == one_layout
    if (multi, one_layout) not in cache:  # the oracle scores the nine distinct queries once per mode, on the device's tables
        cache[(multi, one_layout)] = tp.oracle_dp_on_product_tables(dcp, oracle32, scanner, profiles, queries, multi, False, False)
    on, oa = (x[src] for x in cache[(multi, one_layout)])
    scanner.upload_seqs(seqs)
    scanner.scan(multi, False, 1e30, keep_scores=True, kernel=dcp.KERNEL_QLANE2)
    assert scanner.last_scan_kernel == dcp.KERNEL_QLANE2
    gn, ga = scanner.scores()
    u32 = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    bad = np.argwhere((u32(gn) != u32(on)) | (u32(ga) != u32(oa)))
    if len(bad):
        q, p = int(bad[0][0]), int(bad[0][1])
        raise AssertionError("%d of %d pairs differ; first: query %d (distinct query %d, %d nt) x profile of %d nodes: "
                             "device null %r alt %r, oracle %r %r" % (len(bad), gn.size, q, src[q], len(seqs[q]),
                                                                      profiles[p].core_size, gn[q, p], ga[q, p], on[q, p], oa[q, p]))
