"""The multi-GPU layer for double DBs: `struct dcp_hit64` records (24 bytes, 6 words) through the merge, the
torch.distributed transport and the C library's RCCL gather.

On the CPU: dcp_dist_merge_hits64 against a numpy restatement, score fields as bits; the `[cap, 6]` form of the torch
transport on two gloo ranks; the `[cap, 4]` form still gives float records.  On the GPU: the one-rank RCCL gather of a
double scan's buffer (the meta all-gather and the local-copy leg; RCCL refuses two ranks on one device, so the N > 1
send / recv leg runs nowhere here), shards of a double DB scanned one after the other in one process and merged, and two
gloo ranks sharing the GPU."""
import os
import signal
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 150  # a rank that is stuck ends itself, and with it the test
EVERY = -1e30  # lrt threshold of the float scans here: every finite LRT passes


def words_of(records):
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 6)


def same_bits(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and np.array_equal(words_of(a), words_of(b))


def merge_restated(dtype, counts, offsets, records):
    """What dcp_dist_merge_hits64 says it does: rank r's records get + offsets[r]; stable order by (seq, profile)."""
    out = np.array(records, dtype)
    at = 0
    for n, off in zip(counts, offsets):
        out["profile_idx"][at:at + n] += np.uint32(off)
        at += n
    assert at == len(out)
    return out[np.lexsort((out["profile_idx"], out["seq_idx"]))]  # lexsort is stable


ODD_BITS = np.array([0xFFF0000000000000,   # -inf
                     0x8000000000000000,   # -0.0
                     0x0000000000000001,   # the smallest subnormal
                     0x800FFFFFFFFFFFFF,   # the largest one, negative
                     0x7FF8000000DECAF0,   # a quiet NaN with a payload
                     0xFFF4000000000BAD,   # a signalling one, negative
                     0x7FF0000000000000], np.uint64)


def fabricated(dcp, rng, n, nprof):
    """n records of a shard of nprof profiles, distinct (seq, profile) keys, scores of every kind"""
    h = np.zeros(n, dcp.HIT64_DTYPE)
    keys = rng.permutation(40 * nprof)[:n]
    h["seq_idx"], h["profile_idx"] = keys // nprof, keys % nprof
    for f in ("null_loglik", "alt_loglik"):
        bits = (-rng.random(n) * 1000).view(np.uint64)
        odd = rng.random(n) < 0.4
        bits[odd] = rng.choice(ODD_BITS, int(odd.sum()))
        h[f] = bits.view(np.float64)
    return h


@pytest.mark.parametrize("counts", [[0, 5, 0, 7, 0], [6, 0, 0, 3], [9], [0], [0, 0], [1, 1, 1]])
def test_merge_hits64_against_numpy(dcp, counts):
    """Ranks without records first, last and in the middle, one rank, none at all; -inf, -0.0, subnormals and NaN
    payloads in the score fields come back bit for bit."""
    from deciphon_old_amd import dist as ddist

    assert ddist.HIT64_WORDS == 6 and dcp.HIT64_DTYPE.itemsize == 24
    rng = np.random.default_rng(sum(counts) + len(counts))
    nprof = 30
    offsets = [1000 * r + 17 for r in range(len(counts))]
    parts = [fabricated(dcp, rng, n, nprof) for n in counts]
    records = np.concatenate(parts) if parts else np.zeros(0, dcp.HIT64_DTYPE)
    if sum(counts) >= 6:
        assert len(np.intersect1d(records["null_loglik"].view(np.uint64), ODD_BITS)) >= 1
    got = ddist.merge_hits64(counts, offsets, records)
    assert got.dtype == dcp.HIT64_DTYPE
    assert same_bits(got, merge_restated(dcp.HIT64_DTYPE, counts, offsets, records))
    assert same_bits(ddist.hits64_from_words(words_of(records).view(np.int32)), records)


def test_merge_hits64_order_is_by_seq_then_profile_and_odd_scores_survive(dcp):
    from deciphon_old_amd import dist as ddist

    h = np.zeros(len(ODD_BITS), dcp.HIT64_DTYPE)
    h["seq_idx"] = [5, 5, 0, 9, 0, 2, 5]
    h["profile_idx"] = [3, 1, 8, 0, 2, 2, 0]
    h["null_loglik"], h["alt_loglik"] = ODD_BITS.view(np.float64), ODD_BITS[::-1].view(np.float64)
    got = ddist.merge_hits64([3, 4], [100, 0], h)
    want = merge_restated(dcp.HIT64_DTYPE, [3, 4], [100, 0], h)
    assert same_bits(got, want)
    assert list(zip(got["seq_idx"].tolist(), got["profile_idx"].tolist())) == \
        [(0, 2), (0, 108), (2, 2), (5, 0), (5, 101), (5, 103), (9, 0)]
    assert sorted(got["null_loglik"].view(np.uint64).tolist()) == sorted(ODD_BITS.tolist())


def test_merge_hits64_capacity_and_counts(dcp):
    """A cap one record too small is -1 and writes nothing; counts that do not add up to the records raise."""
    from deciphon_old_amd import dist as ddist

    rng = np.random.default_rng(3)
    rec = fabricated(dcp, rng, 7, 10)
    counts, offs = np.array([3, 4], np.uint32), np.array([0, 10], np.uint32)
    out = np.zeros(8, dcp.HIT64_DTYPE)
    out["seq_idx"] = 0xDEAD
    merge = dcp.lib.dcp_dist_merge_hits64
    assert merge(counts.ctypes.data, offs.ctypes.data, 2, rec.ctypes.data, out.ctypes.data, 6) == -1
    assert (out["seq_idx"] == 0xDEAD).all()
    assert merge(counts.ctypes.data, offs.ctypes.data, 2, rec.ctypes.data, out.ctypes.data, 7) == 7
    assert same_bits(out[:7], merge_restated(dcp.HIT64_DTYPE, [3, 4], [0, 10], rec)) and out["seq_idx"][7] == 0xDEAD
    assert merge(None, offs.ctypes.data, 2, rec.ctypes.data, out.ctypes.data, 7) == -1
    assert merge(counts.ctypes.data, offs.ctypes.data, 0, rec.ctypes.data, out.ctypes.data, 7) == -1
    for bad_counts, bad_offs in (([3, 3], [0, 10]), ([3, 5], [0, 10]), ([3, 4], [0]), ([7], [0, 10])):
        with pytest.raises(dcp.DcpError):
            ddist.merge_hits64(bad_counts, bad_offs, rec)
    # float records are not double ones
    with pytest.raises((dcp.DcpError, TypeError, ValueError)):
        ddist.merge_hits64([7], [0], np.zeros(7, dcp.HIT_DTYPE))


def _product():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_product

    dcp = load_product()
    from deciphon_old_amd import dist as ddist
    return dcp, ddist


def _cpu_worker(rank, world, port, tmpdir):
    signal.alarm(CHILD_SECONDS)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dcp, ddist = _product()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bounds = [(0, 40), (40, 95)]
        b = bounds[rank][0]

        def local_hits(r, n):
            return fabricated(dcp, np.random.default_rng(640 + r), n, bounds[r][1] - bounds[r][0])

        cap = 64
        for counts in ([3, 5], [0, 4], [6, 0], [0, 0], [40, 2]):  # a rank that holds nothing; more than one slab
            n = counts[rank]
            words = torch.zeros((cap, 6), dtype=torch.int32)
            if n:
                words[:n] = torch.from_numpy(words_of(local_hits(rank, n)).view(np.int32).copy())
            got = ddist.gather_hits(words, torch.tensor([n], dtype=torch.int32), b, slab=8)
            parts = [local_hits(r, counts[r]) for r in range(world)]
            want = ddist.merge_hits64(counts, [x for x, _ in bounds], np.concatenate(parts))
            assert got.dtype == dcp.HIT64_DTYPE and len(got) == sum(counts)
            assert same_bits(got, want)
            assert same_bits(got, merge_restated(dcp.HIT64_DTYPE, counts, [x for x, _ in bounds], np.concatenate(parts)))
            again = ddist.gather_hits64(words, torch.tensor([n], dtype=torch.int32), b, slab=8)
            assert same_bits(again, want)
            # both ranks hold the same list
            mine = torch.from_numpy(words_of(got).view(np.int32).copy()) if len(got) else torch.zeros((0, 6), dtype=torch.int32)
            lists = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(lists, mine)
            assert all(torch.equal(t, mine) for t in lists)
        # one rank found more than its buffer holds: BOTH raise, neither returns a short list
        for found in ([9, 2], [2, 9], [4, 5]):
            try:
                ddist.gather_hits(torch.zeros((4, 6), dtype=torch.int32), torch.tensor([found[rank]], dtype=torch.int32), b)
                raise AssertionError(f"rank {rank}: the overflow {found} went unnoticed")
            except RuntimeError:
                pass
        # gather_hits64 takes 6-word records only
        try:
            ddist.gather_hits64(torch.zeros((4, 4), dtype=torch.int32), torch.tensor([0], dtype=torch.int32), b)
            raise AssertionError("4-word records taken for dcp_hit64")
        except (ValueError, dcp.DcpError):
            pass
        # the float transport is what it was: [cap, 4] words come back as HIT_DTYPE
        f = np.zeros(3, dcp.HIT_DTYPE)
        f["seq_idx"], f["profile_idx"] = [2, 0, 1], [1, 2, 0]
        f["null_loglik"], f["alt_loglik"] = [-3.5, -np.inf, -0.0], [-1.25, 7.0, 2.5]
        n = (3, 1)[rank]
        words = torch.zeros((8, 4), dtype=torch.int32)
        words[:n] = torch.from_numpy(f[:n].view(np.int32).reshape(n, 4).copy())
        got = ddist.gather_hits(words, torch.tensor([n], dtype=torch.int32), b)
        want = ddist.merge_hits([3, 1], [0, 40], np.concatenate([f, f[:1]]))
        assert got.dtype == dcp.HIT_DTYPE and len(got) == 4
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert list(zip(got["seq_idx"].tolist(), got["profile_idx"].tolist())) == [(0, 2), (1, 0), (2, 1), (2, 41)]
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def spawn_ranks(worker, world, port, tmpdir):
    """The ranks as fresh processes; what is still running at the deadline is killed."""
    ctx = mp.spawn(worker, args=(world, port, tmpdir), nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_SECONDS + 20
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "a rank did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


def test_gather_hits_transport_with_six_word_records_world2(tmp_path):
    world = 2
    spawn_ranks(_cpu_worker, world, 30100 + (os.getpid() % 1000), str(tmp_path))
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


# ---- GPU ---------------------------------------------------------------------------------------------------------


def gpu_world(sharded=False):
    """test_f64_hit_buffer's DB and batch.  sharded: nothing planted in the last profile, which is a shard of its own
    when the DB is cut in three -- a rank without a hit."""
    from oracle_py import Oracle
    from test_f64_hit_buffer import PLANTED, SIZES, build_world

    dcp, ddist = _product()
    planted = {q: p for q, p in PLANTED.items() if not (sharded and p == len(SIZES) - 1)}
    if sharded:
        assert ddist.shard_range(SIZES, 3, 2) == (len(SIZES) - 1, len(SIZES)) and len(planted) == len(PLANTED) - 1
    profs, seqs = build_world(dcp, Oracle(64), planted=planted)
    return SIZES, profs, seqs


@pytest.mark.gpu
def test_c_rccl_gather_one_rank_in_double(dcp):
    """test_c_rccl_gather_one_rank's twin: the double scan's buffer through ncclCommInitRank(1 rank), the 3-word
    all-gather, the local-copy leg of the gather-v and dcp_dist_merge_hits64 -- with a float gather before and after it
    on the same communicator."""
    from deciphon_old_amd import dist as ddist

    sizes, profs, seqs = gpu_world()
    fprofs = [dcp.ProteinProfile.sample(11 + i, M) for i, M in enumerate((30, 64, 90))]
    sc, fsc = dcp.Scanner(0), dcp.Scanner(0)
    comm = ddist.CDist.create(ddist.CDist.unique_id(), 0, 1, 0)
    times = {}
    try:
        fsc.upload_db(fprofs)
        fsc.upload_seqs(seqs)
        fsc.scan(True, False, EVERY)
        fwant = fsc.hits().copy()
        assert len(fwant) >= 2
        fsc.scan(True, False, EVERY, sync=False)
        got, total = comm.gather_scan_hits(fsc, 0)
        times["float"] = comm.last_gather_ms
        assert total == len(fwant) and got.dtype == dcp.HIT_DTYPE and np.array_equal(got.view(np.uint32), fwant.view(np.uint32))

        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        sc.scan(True, False, 10.0)
        want = sc.hits().copy()
        assert len(want) >= 4
        cap = 1024
        hits_dev = torch.zeros((cap, 6), dtype=torch.int32, device="cuda")
        count_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        sc.set_hit_buffer64(hits_dev.data_ptr(), cap, count_dev.data_ptr())
        sc.scan(True, False, 10.0, sync=False)
        for root in (-1, 0):
            got, total = comm.gather_hits64(hits_dev.data_ptr(), count_dev.data_ptr(), cap, 0, sc.stream, root=root)
            assert total == len(want) and got.dtype == dcp.HIT64_DTYPE and same_bits(got, want)
        times["double"] = comm.last_gather_ms
        # a shard that does not start at profile 0: indices come back global, the scores as they were
        got, _ = comm.gather_hits64(hits_dev.data_ptr(), count_dev.data_ptr(), cap, 1000, sc.stream)
        shifted = want.copy()
        shifted["profile_idx"] += 1000
        assert same_bits(got, shifted)
        # the form hosts call, after either kernel: the gather completes the scan itself
        for kernel in (dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE64):
            sc.scan(True, False, 10.0, sync=False, kernel=kernel)
            got, total = comm.gather_scan_hits64(sc, 0)
            assert total == len(want) and same_bits(got, want), kernel
            assert sc.last_scan_kernel == kernel and int(count_dev.cpu()[0]) == len(want)
        # a buffer too small for the scan's hits: DCP_ENOMEM, not a short list taken for the whole
        sc.set_hit_buffer64(hits_dev.data_ptr(), 1, count_dev.data_ptr())
        sc.scan(True, False, 10.0, sync=False)
        with pytest.raises(dcp.DcpError) as ei:
            comm.gather_scan_hits64(sc, 0)
        assert ei.value.rc == dcp.RC_ENOMEM
        sc.set_hit_buffer64(None, 0, None)
        # without a caller buffer the context's own one is gathered
        sc.scan(True, False, 10.0, sync=False, kernel=dcp.KERNEL_QLANE64)
        got, _ = comm.gather_scan_hits64(sc, 0)
        assert same_bits(got, want)
        assert comm.comm_count == 1 and comm.last_gather_ms > 0.0
        # a context that never scanned, and one whose last scan was float, hold no dcp_hit64 records: they complete both
        # exchanges marked DCP_DIST_FOUND_FAILED and return the context's own error
        never = dcp.Scanner(0)
        try:
            with pytest.raises(dcp.DcpError) as ei:
                comm.gather_scan_hits64(never, 0)
            assert ei.value.rc == dcp.RC_EINVAL and "no scan yet" in str(ei.value)
        finally:
            never.close()
        with pytest.raises(dcp.DcpError) as ei:
            comm.gather_scan_hits64(fsc, 0)
        assert ei.value.rc == dcp.RC_EINVAL and "float DB" in str(ei.value)
        with pytest.raises(dcp.DcpError) as ei:  # and the float gather refuses the double scan as before
            comm.gather_scan_hits(sc, 0)
        assert ei.value.rc == dcp.RC_EINVAL and "dcp_hit64" in str(ei.value)
        got, _ = comm.gather_scan_hits64(sc, 0)  # the communicator is still usable
        assert same_bits(got, want)
        fsc.scan(True, False, EVERY, sync=False)
        got, total = comm.gather_scan_hits(fsc, 0)
        assert total == len(fwant) and got.dtype == dcp.HIT_DTYPE and np.array_equal(got.view(np.uint32), fwant.view(np.uint32))
        print("one-rank gather, last_gather_ms: double %.3f (%d records), float %.3f (%d records)"
              % (times["double"], len(want), times["float"], len(fwant)))
    finally:
        comm.close()
        sc.close()
        fsc.close()


def scan_shard(dcp, ddist, sizes, profs, seqs, world, rank, cap=256):
    """Rank `rank` of `world`: its shard resident, all queries scanned by kernel 4 into a caller buffer.
    Returns (begin, end, the records held as [n, 6] int32 words on the device's side copied out, null, alt)."""
    b, e = ddist.shard_range(sizes, world, rank)
    hits_dev = torch.zeros((cap, 6), dtype=torch.int32, device="cuda")
    count_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    sc = dcp.Scanner(0)
    try:
        sc.upload_db(profs[b:e])
        sc.upload_seqs(seqs)
        sc.set_hit_buffer64(hits_dev.data_ptr(), cap, count_dev.data_ptr())
        sc.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE64)
        assert sc.last_scan_kernel == dcp.KERNEL_QLANE64
        nl, al = sc.scores()
    finally:
        sc.close()
    n = int(count_dev.cpu()[0])
    assert n <= cap
    return b, e, hits_dev, count_dev, n, nl, al


def unsharded(dcp, profs, seqs):
    full = dcp.Scanner(0)
    try:
        full.upload_db(profs)
        full.upload_seqs(seqs)
        full.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE64)
        return full.hits().copy(), full.scores()
    finally:
        full.close()


@pytest.mark.gpu
def test_shards_equal_the_whole(dcp):
    """World sizes 2 and 3 in one process: every rank's shard scanned into a caller buffer, the held records merged by
    dcp_dist_merge_hits64 -- the unsharded scan's list record for record, as bits; one shard of three has no hit."""
    from deciphon_old_amd import dist as ddist

    sizes, profs, seqs = gpu_world(sharded=True)
    want, (fn, fa) = unsharded(dcp, profs, seqs)
    assert len(want) >= 4
    empty_shards = 0
    for world in (2, 3):
        counts, offs, parts = [], [], []
        for rank in range(world):
            b, e, hits_dev, _, n, nl, al = scan_shard(dcp, ddist, sizes, profs, seqs, world, rank)
            assert np.array_equal(nl.view(np.uint64), fn[:, b:e].view(np.uint64))
            assert np.array_equal(al.view(np.uint64), fa[:, b:e].view(np.uint64))
            counts.append(n)
            offs.append(b)
            parts.append(ddist.hits64_from_words(hits_dev[:n].cpu().numpy()))
            empty_shards += n == 0
        assert offs[0] == 0 and sum(counts) == len(want)
        assert same_bits(ddist.merge_hits64(counts, offs, np.concatenate(parts)), want)
    assert empty_shards == 1  # the third of three


def _gpu_worker(rank, world, port, tmpdir):
    """Two ranks share the one GPU: each holds its shard of the double DB resident, scans ALL queries into a [256, 6]
    device tensor, and the records are all-gathered through the [cap, 6] transport."""
    signal.alarm(CHILD_SECONDS)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dcp, ddist = _product()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sizes, profs, seqs = gpu_world(sharded=True)
        b, e, hits_dev, count_dev, n, nl, al = scan_shard(dcp, ddist, sizes, profs, seqs, world, rank)
        assert tuple(hits_dev.shape) == (256, 6)
        allh = ddist.gather_hits(hits_dev.cpu(), count_dev.cpu(), b)
        assert allh.dtype == dcp.HIT64_DTYPE
        if rank == 0:  # the unsharded scan gives the same hit list, record for record
            want, (fn, fa) = unsharded(dcp, profs, seqs)
            assert len(want) >= 4 and same_bits(allh, want)
            assert np.array_equal(nl.view(np.uint64), fn[:, b:e].view(np.uint64))
            assert np.array_equal(al.view(np.uint64), fa[:, b:e].view(np.uint64))
        open(os.path.join(tmpdir, f"gpu_ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_double_scan_two_ranks_one_gpu(tmp_path):
    world = 2
    spawn_ranks(_gpu_worker, world, 31300 + (os.getpid() % 1000), str(tmp_path))
    assert all((tmp_path / f"gpu_ok{r}").exists() for r in range(world))
