"""The random batch: dcp_seq_random_thresholds / dcp_seq_random on the host (csrc/dcp_model.cpp) and random_words_kernel
(csrc/dcp_calib.hip) behind dcp_gpu_seqs_random / Scanner.random_seqs on the device.  The rule is integer arithmetic
mod 2^64 (csrc/dcp_calib.h): every comparison here is in bits.

CPU: the generator against a Python restatement of the rule, the thresholds, the refusals, base frequencies.
GPU:
  1. every word of a random batch against the host packing of dcp_seq_random, pad words and tail bits included, and
     fetch_seq; add_reverse_strand and cut_windows behind a random batch against the same sequences uploaded by hand;
  2. the refusals, with the previous batch intact;
  3. a random batch scans to the bits of the same sequences uploaded by hand, on every kernel."""
import numpy as np
import pytest

from test_both_strands import bits, hit_fields, host_words, np_revcomp
from test_seq_windows import hand_cut

M64 = (1 << 64) - 1
SEEDS = (0, 1, 7, 0x9E3779B97F4A7C15, M64)
LENGTHS = (1, 3, 4, 5, 16, 17, 1000)
SKEW = (0.1, 0.4, 0.0, 0.5)


def sm(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_thresholds(probs):
    if probs is None:
        return [16384, 32768, 49152]
    cum, out = 0.0, []
    for p in probs[:3]:
        cum += p
        out.append(min(int(np.floor(65536.0 * cum + 0.5)), 65536))
    return out


def py_random(seed, q, length, probs=None):
    """the rule as stated, base by base"""
    c = py_thresholds(probs)
    key = sm(seed ^ sm(q))
    out = np.zeros(length, np.uint8)
    for b in range(length):
        u = (sm((key + (b >> 2)) & M64) >> (16 * (b & 3))) & 0xffff
        out[b] = (u >= c[0]) + (u >= c[1]) + (u >= c[2])
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------


def test_generator_equals_the_restatement(dcp):
    for probs in (None, SKEW):
        for seed in SEEDS:
            for q in (0, 1, 2 ** 32 - 1):
                for L in LENGTHS:
                    got = dcp.random_seq(seed, q, L, probs)
                    assert got.dtype == np.uint8 and np.array_equal(got, py_random(seed, q, L, probs)), (probs, seed, q, L)


def test_a_shorter_sequence_is_a_prefix_and_sequences_differ(dcp):
    long = dcp.random_seq(7, 3, 1000)
    for L in LENGTHS:
        assert np.array_equal(dcp.random_seq(7, 3, L), long[:L])
    assert not np.array_equal(dcp.random_seq(7, 4, 1000), long) and not np.array_equal(dcp.random_seq(8, 3, 1000), long)


def test_thresholds(dcp):
    assert dcp.random_thresholds().tolist() == [16384, 32768, 49152]
    assert dcp.random_thresholds((0.25, 0.25, 0.25, 0.25)).tolist() == [16384, 32768, 49152]
    assert dcp.random_thresholds(SKEW).tolist() == [6554, 32768, 32768]
    assert dcp.random_thresholds((1, 0, 0, 0)).tolist() == [65536, 65536, 65536]
    assert dcp.random_thresholds((0, 0, 0, 1)).tolist() == [0, 0, 0]
    rng = np.random.default_rng(3)
    for _ in range(200):
        p = rng.dirichlet(np.ones(4))
        assert dcp.random_thresholds(p).tolist() == py_thresholds(list(p)), p


def test_skewed_and_degenerate_compositions(dcp):
    s = dcp.random_seq(5, 0, 20000, SKEW)
    assert not (s == 2).any() and (s == 0).any() and (s == 1).any() and (s == 3).any()  # no G ever appears
    assert np.array_equal(s, py_random(5, 0, 20000, SKEW))
    for seed in SEEDS:
        assert not dcp.random_seq(seed, 2 ** 32 - 1, 1000, (1, 0, 0, 0)).any()
        assert (dcp.random_seq(seed, 0, 1000, (0, 0, 0, 1)) == 3).all()


def test_refusals(dcp):
    nan, inf = float("nan"), float("inf")
    for bad in ((0.5, 0.5, 0.5, 0.5), (0.25, 0.25, 0.25, 0.2), (1.5, -0.5, 0, 0), (nan, 0.5, 0.25, 0.25), (inf, 0, 0, 0),
                (0.25, 0.25, 0.25, 0.25 + 2e-6), (0, 0, 0, 0)):
        with pytest.raises(dcp.DcpError) as e:
            dcp.random_thresholds(bad)
        assert e.value.rc == dcp.RC_EINVAL, bad
        with pytest.raises(dcp.DcpError):
            dcp.random_seq(1, 0, 10, bad)
        c = np.full(3, 9, np.uint32)
        assert dcp.lib.dcp_seq_random_thresholds(np.array(bad, np.float64).ctypes.data, c.ctypes.data) == dcp.RC_EINVAL
        assert (c == 9).all()
    assert dcp.random_thresholds((0.25, 0.25, 0.25, 0.25 + 5e-7)).tolist() == [16384, 32768, 49152]  # inside 1e-6
    assert dcp.lib.dcp_seq_random_thresholds(None, None) == dcp.RC_EINVAL
    with pytest.raises(dcp.DcpError):
        dcp.random_thresholds((0.5, 0.5))
    assert len(dcp.random_seq(1, 0, 0)) == 0


def test_base_frequencies(dcp):
    """Sanity that hides nothing: the restatement gives 0.2481 .. 0.2514 for these 200 000 bases."""
    s = dcp.random_seq(1, 0, 200000)
    f = np.bincount(s, minlength=4) / len(s)
    print("base frequencies of (seed 1, q 0), 200 000 bases:", f)
    assert (f > 0.245).all() and (f < 0.255).all(), f
    assert np.array_equal(s[:5000], py_random(1, 0, 5000))


# ---- GPU: words --------------------------------------------------------------------------------------------------

BATCHES = ((1, 1), (1, 15), (3, 16), (64, 17), (65, 31), (2, 32), (2, 33), (300, 100), (5, 1000))


def host_batch(dcp, n, L, seed, probs=None):
    return [dcp.random_seq(seed, q, L, probs) for q in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("probs", [None, SKEW], ids=["uniform", "skewed"])
def test_every_word_of_a_random_batch(dcp, probs):
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    for k, (n, L) in enumerate(BATCHES):
        seed = SEEDS[k % len(SEEDS)]
        sc.random_seqs(n, L, seed, probs)  # no DB resident
        assert (sc.nseqs, sc.strands, sc.windows, sc.regions) == (n, 1, None, 0)
        want = host_batch(dcp, n, L, seed, probs)
        for q in range(n):
            got = sc.test_seq_words(q)
            assert np.array_equal(got, host_words(want[q])), (n, L, q, [hex(x) for x in got])
            assert np.array_equal(sc.fetch_seq(q), want[q]), (n, L, q)
        if probs is not None:
            assert not any((s == 2).any() for s in want)
    sc.close()


@pytest.mark.gpu
def test_reverse_strand_and_windows_behind_a_random_batch(dcp):
    a, b = dcp.Scanner(0, lib=dcp.load_testhooks()), dcp.Scanner(0, lib=dcp.load_testhooks())
    n, L, seed = 37, 100, 11
    seqs = host_batch(dcp, n, L, seed)
    a.random_seqs(n, L, seed)
    a.add_reverse_strand()
    b.upload_seqs(seqs + [np_revcomp(s) for s in seqs])
    assert a.nseqs == b.nseqs == 2 * n and a.strands == 2
    for q in range(2 * n):
        assert np.array_equal(a.test_seq_words(q), b.test_seq_words(q)), q
    a.random_seqs(n, L, seed)
    a.cut_windows(33, 17)
    cut = hand_cut(seqs, 33, 17)
    b.upload_seqs(cut)
    assert a.nseqs == b.nseqs == len(cut) and a.windows == (33, 17)
    for q in range(len(cut)):
        assert np.array_equal(a.test_seq_words(q), b.test_seq_words(q)), q
    a.add_reverse_strand()
    assert np.array_equal(a.fetch_seq(len(cut) + 5), np_revcomp(cut[5]))
    # regions too, and the next random batch returns the context to uncut
    a.random_seqs(n, L, seed)
    a.cut_regions([3, 36], [10, 0], [50, 100], [0, 1])
    assert np.array_equal(a.fetch_seq(0), seqs[3][10:60]) and np.array_equal(a.fetch_seq(1), np_revcomp(seqs[36]))
    a.random_seqs(2, 5, seed)
    assert (a.nseqs, a.strands, a.windows, a.regions) == (2, 1, None, 0)
    a.close()
    b.close()


@pytest.mark.gpu
def test_refusals_leave_the_batch_intact(dcp):
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    seqs = host_batch(dcp, 5, 40, 3)
    sc.upload_seqs(seqs)
    sc.cut_windows(16, 16)
    state = (sc.nseqs, sc.strands, sc.windows)
    words = [sc.test_seq_words(q) for q in range(sc.nseqs)]
    uniform = np.full(4, 0.25)
    calls = {
        "no sequences": (0, 10, uniform), "no bases": (10, 0, uniform), "probs": (10, 10, np.array([0.5, 0.5, 0.5, 0.5])),
        "nan": (10, 10, np.array([np.nan, 0.5, 0.25, 0.25])),
        "words": (2 ** 31, 16, uniform),          # 2^31 x 4 words
        "three words": (1431655766, 1, uniform),  # 3 n = 2^32 + 2
        "long": (16, 2 ** 32 - 1, uniform),       # 16 x (2^28 + 2)
    }
    for name, (n, L, p) in calls.items():
        rc = sc._lib.dcp_gpu_seqs_random(sc._c, n, L, 1, p.ctypes.data)
        assert rc == dcp.RC_EINVAL, name
        assert sc._lib.dcp_gpu_last_error(sc._c), name
        assert (sc.nseqs, sc.strands, sc.windows) == state, name
    for q in range(sc.nseqs):
        assert np.array_equal(sc.test_seq_words(q), words[q]), q
    with pytest.raises(dcp.DcpError) as e:
        sc.random_seqs(0, 10, 1)
    assert e.value.rc == dcp.RC_EINVAL and "random batch" in str(e.value)
    sc.close()


# ---- GPU: the bits of a batch uploaded by hand -------------------------------------------------------------------

SAME_BITS_CASES = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 4)]  # (precision, dcp_scan_params.kernel)
SCAN_M = (3, 64, 65, 130)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,kernel", SAME_BITS_CASES)
def test_same_bits_as_the_sequences_uploaded_by_hand(dcp, precision, kernel):
    cfg = dcp.ProteinCfg(2, 0.01)
    profs = [dcp.ProteinProfile.sample(100 + M, M, cfg, f"R{M}", precision=precision) for M in SCAN_M]
    n, L, seed = 70, 60, 21
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    a.random_seqs(n, L, seed)
    b.upload_seqs(host_batch(dcp, n, L, seed))
    assert a.cells == b.cells and a.algorithmic_bytes == b.algorithmic_bytes
    for multi_hits in (False, True):
        a.scan(multi_hits, False, 0.0, kernel=kernel)
        b.scan(multi_hits, False, 0.0, kernel=kernel)
        for x, y in zip(a.scores(), b.scores()):
            assert np.isfinite(x).all() and np.array_equal(bits(x), bits(y)), (precision, kernel, multi_hits)
        assert hit_fields(a.hits()) == hit_fields(b.hits())
        assert a.last_scan_kernel == b.last_scan_kernel == kernel
    a.close()
    b.close()
