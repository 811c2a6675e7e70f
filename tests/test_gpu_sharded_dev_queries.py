"""bivx_query_sharded_dev_q: a sharded handle answers a batch whose queries are already in devices[0]'s memory. The queries
are routed to their chromosomes' devices by kernels on devices[0] (route.hip); with batch_order the gathered CSR is put back
into batch order on the device. The test box has one GPU, so most handles name device 0 several times: the routing, the
in-place blocks, the gather and the permutation are the same as on a node; only the RCCL branch needs two cards."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNHELD = 5  # a chromosome id inside the table whose intervals are left out of the index


def _to(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to("cuda:0")


def _genome(n, q, seed):
    from binary_amd import synth
    d = synth.gen_genome(n, q, 1000)
    keep = d["chrom"] != UNHELD
    for key in ("chrom", "low", "high"):
        d[key] = d[key][keep]
    perm = np.random.default_rng(seed).permutation(d["qlow"].size)
    for key in ("qchrom", "qlow", "qhigh"):
        d[key] = np.ascontiguousarray(d[key][perm])
    return d


def _built(devices, d, chrom=True):
    from binary_amd import IntervalIndex
    idx = IntervalIndex(devices)
    idx.insert_node(d["low"], d["high"], d["chrom"] if chrom else None)
    idx.build()
    return idx


def _single(one, qlo, qhi, qc, sort_by_id):
    """bivx_query_dev_s of a single index: the canonical CSR"""
    import torch
    if qlo.size == 0:
        return torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.zeros(0, dtype=torch.int32, device="cuda:0")
    c = None if qc is None else _to(qc)
    off = one.count_overlaps_device(_to(qlo), _to(qhi), c)
    hits = torch.empty(int(off[-1].item()), dtype=torch.int32, device="cuda:0")
    one.query_device(_to(qlo), _to(qhi), off, hits, qchrom=c, sort_by_id=sort_by_id)
    torch.cuda.synchronize()
    return off, hits


def _dev_q(sh, qlo, qhi, qc, sort_by_id, batch_order):
    return sh.query_sharded_device_tensors(_to(qlo), _to(qhi), None if qc is None else _to(qc), sort_by_id=sort_by_id,
                                           batch_order=batch_order)


def _lists(off, hits, rows, q):
    off, hits = off.cpu().numpy(), hits.cpu().numpy()
    rows = np.arange(q) if rows is None else rows.cpu().numpy()
    assert rows.size == q and np.array_equal(np.sort(rows), np.arange(q))
    out = [None] * q
    for r, qi in enumerate(rows):
        out[qi] = hits[off[r]:off[r + 1]]
    return out


def _lpt(chrom, k):
    """the handle's chromosome -> shard assignment (sharded.cpp, build_impl)"""
    cnt = np.bincount(chrom)
    order = sorted([c for c in range(cnt.size) if cnt[c]], key=lambda c: -(cnt[c] * np.log2(cnt[c] + 2.0)))
    load, shard = [0.0] * k, {}
    for c in order:
        s = int(np.argmin(load))
        shard[c] = s
        load[s] += cnt[c] * np.log2(cnt[c] + 2.0)
    return shard


def _assert_same(a, b):
    import torch
    assert a[0].dtype == b[0].dtype and torch.equal(a[0], b[0]), "offsets"
    assert torch.equal(a[1], b[1]), "ids"


@pytest.mark.parametrize("sort_by_id", [False, True])
@pytest.mark.parametrize("batch_order", [False, True])
def test_one_device_equals_the_single_index_bit_for_bit(sort_by_id, batch_order):
    import torch
    d = _genome(400_000, 250_000, 3)
    qc = d["qchrom"].copy()
    qc[:50] = 77                                         # nobody holds chromosome 77: empty rows
    with _built(0, d) as one, _built([0], d) as sh:
        exp = _single(one, d["qlow"], d["qhigh"], qc, sort_by_id)
        off, hits, rows, used_rccl = _dev_q(sh, d["qlow"], d["qhigh"], qc, sort_by_id, batch_order)
        assert used_rccl
        _assert_same((off, hits), exp)
        if batch_order:
            assert rows is None
        else:
            assert torch.equal(rows, torch.arange(qc.size, dtype=torch.int32, device="cuda:0"))


@pytest.mark.parametrize("sort_by_id", [False, True])
def test_three_shards_by_chromosome(sort_by_id):
    import torch
    d = _genome(300_000, 200_000, 4)
    qc = d["qchrom"].copy()
    qc[::997] = 24                                       # just beyond the table
    qc[5::1009] = 31
    qc[7::1013] = 0xFFFFFFFF
    assert (qc == UNHELD).any()                          # inside the table, no interval
    qlo, qhi = d["qlow"], d["qhigh"]
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=sort_by_id)
        dev = _dev_q(sh, qlo, qhi, qc, sort_by_id, False)
        # the device routing is the host routing: a stable partition, unheld chromosomes merged into shard 0
        for a, b in zip(host[:3], dev[:3]):
            assert torch.equal(a, b)
        assert not dev[3]
        r = dev[2].cpu().numpy()
        assert not np.array_equal(r, np.arange(r.size))  # (the rows really are grouped: the permutation below has work)
        off, hits, rows, _ = _dev_q(sh, qlo, qhi, qc, sort_by_id, True)
        assert rows is None and off.numel() == qlo.size + 1
        if sort_by_id:
            _assert_same((off, hits), _single(one, qlo, qhi, qc, True))
        else:                                            # index order of a shard: the host-input call's lists
            got, exp = _lists(off, hits, None, qlo.size), _lists(*host[:3], qlo.size)
            assert all(np.array_equal(a, b) for a, b in zip(got, exp))


@pytest.mark.parametrize("batch_order", [False, True])
def test_replicated_handle_splits_the_device_columns(batch_order):
    import torch
    from binary_amd import IntervalIndex, synth
    low, high = synth.gen_intervals(100_000, 30_000_000, 2000)
    qlo, qhi = synth.gen_range_queries(50_001, 30_000_000, 2000)
    with IntervalIndex(0) as one, IntervalIndex([0, 0, 0]) as rep:
        for idx in (one, rep):
            idx.insert_node(low, high)
            idx.build()
        exp = _single(one, qlo, qhi, None, True)
        off, hits, rows, _ = _dev_q(rep, qlo, qhi, None, True, batch_order)
        _assert_same((off, hits), exp)
        assert rows is None if batch_order else torch.equal(rows.cpu(), torch.arange(qlo.size, dtype=torch.int32))


@pytest.mark.parametrize("q", [0, 1, 8191, 8193])
def test_batch_sizes_around_a_routing_tile(q):
    d = _genome(200_000, 100_000, 5)
    qc, qlo, qhi = d["qchrom"][:q], d["qlow"][:q], d["qhigh"][:q]
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        exp = _single(one, qlo, qhi, qc, True)
        for batch_order in (False, True):
            off, hits, rows, _ = _dev_q(sh, qlo, qhi, qc, True, batch_order)
            if batch_order:
                _assert_same((off, hits), exp)
            else:
                host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=True)
                _assert_same((off, hits), host)
                assert np.array_equal(rows.cpu().numpy(), host[2].cpu().numpy())


def test_large_batch_takes_the_pipelined_kernel_on_every_shard():
    from binary_amd import IntervalIndex
    import torch
    d = _genome(4_000_000, 4_000_000, 6)
    qc, qlo, qhi = d["qchrom"], d["qlow"], d["qhigh"]
    shard = _lpt(d["chrom"], 3)
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        exp = _single(one, qlo, qhi, qc, True)
        cnt = np.diff(exp[0].cpu().numpy())
        tab = np.zeros(24, np.int64)
        for c, v in shard.items():
            tab[c] = v
        qs = tab[qc]                                     # (chromosome 5 is nobody's: shard 0)
        for s in range(3):                               # every shard's batch is one the pipelined kernel takes
            sel = np.isin(d["chrom"], [c for c, v in shard.items() if v == s])
            with IntervalIndex(0) as part:
                part.insert_node(d["low"][sel], d["high"][sel], d["chrom"][sel])
                part.build()
                m, h = int((qs == s).sum()), int(cnt[qs == s].sum())
                assert part.query_kernel_name(m, h, True) == "k_query_pipe", (s, m, h)
        off, hits, rows, _ = _dev_q(sh, qlo, qhi, qc, True, True)
        _assert_same((off, hits), exp)
        host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=True)
        dev = _dev_q(sh, qlo, qhi, qc, True, False)
        for a, b in zip(host[:3], dev[:3]):
            assert torch.equal(a, b)


def test_every_query_on_one_shard():
    d = _genome(300_000, 200_000, 7)
    shard = _lpt(d["chrom"], 3)
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        for s in (0, 2):                                 # the first shard (rows already in batch order) and the last
            sel = np.isin(d["qchrom"], [c for c, v in shard.items() if v == s])
            qc, qlo, qhi = d["qchrom"][sel], d["qlow"][sel], d["qhigh"][sel]
            exp = _single(one, qlo, qhi, qc, True)
            _assert_same(_dev_q(sh, qlo, qhi, qc, True, True)[:2], exp)
            off, hits, rows, _ = _dev_q(sh, qlo, qhi, qc, True, False)
            host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=True)
            _assert_same((off, hits), host)
            assert np.array_equal(rows.cpu().numpy(), np.arange(qc.size))


def test_columns_written_on_a_side_stream_just_before_the_call():
    import torch
    d = _genome(300_000, 400_000, 8)
    qc, qlo, qhi = d["qchrom"], d["qlow"], d["qhigh"]
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        exp = _single(one, qlo, qhi, qc, True)
        src = [_to(x) for x in (qlo, qhi, qc)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            m = torch.rand(2048, 2048, device="cuda:0")
            for _ in range(8):                           # work in front of the writes on the same stream
                m = torch.tanh(m @ m)
            cols = [torch.empty_like(x) for x in src]
            for dst, x in zip(cols, src):
                dst.copy_(x)
            off, hits, rows, _ = sh.query_sharded_device_tensors(cols[0], cols[1], cols[2], sort_by_id=True, batch_order=True)
        torch.cuda.synchronize()
        _assert_same((off, hits), exp)


def test_host_and_device_calls_interleave_on_one_handle():
    d = _genome(300_000, 300_000, 9)
    qc, qlo, qhi = d["qchrom"], d["qlow"], d["qhigh"]
    small = slice(0, 60_000)
    with _built(0, d) as one, _built([0, 0, 0], d) as sh:
        exp = _single(one, qlo[small], qhi[small], qc[small], True)
        h1 = sh.query_sharded_device(qlo[small], qhi[small], qc[small], sort_by_id=True)
        d1 = _dev_q(sh, qlo[small], qhi[small], qc[small], True, True)
        h2 = sh.query_sharded_device(qlo[small], qhi[small], qc[small], sort_by_id=True)
        for a, b in zip(h1[:3], h2[:3]):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        _assert_same(d1[:2], exp)
        more = _genome(500_000, 10, 10)                  # a rebuild, then a larger batch: the handle's buffers grow
        for idx in (one, sh):
            idx.insert_node(more["low"], more["high"], more["chrom"])
            idx.build()
        exp = _single(one, qlo, qhi, qc, True)
        _assert_same(_dev_q(sh, qlo, qhi, qc, True, True)[:2], exp)
        host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=True)
        _assert_same(_dev_q(sh, qlo, qhi, qc, True, False)[:2], host)


def test_errors():
    from binary_amd import IntervalIndex, capi
    q = np.array([5, 9], np.uint32)
    dq = _to(q)
    with IntervalIndex(0) as one:
        one.insert_node(q, q)
        one.build()
        with pytest.raises(capi.BivxError) as e:
            one.query_sharded_device_tensors(dq, dq)
        assert e.value.code == capi.E_STATE
    with IntervalIndex([0, 0]) as sh:
        sh.insert_node(q, q)
        with pytest.raises(capi.BivxError) as e:
            sh.query_sharded_device_tensors(dq, dq)
        assert e.value.code == capi.E_STATE
        sh.build()
        res = capi.ShardedResult()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        vp = lambda t: C.c_void_p(t.data_ptr())
        assert sh._L.bivx_query_sharded_dev_q(sh._h, None, p(q), vp(dq), 2, 1, 1, C.byref(res), None) == capi.E_INVALID
        assert sh._L.bivx_query_sharded_dev_q(sh._h, None, vp(dq), p(q), 2, 1, 0, C.byref(res), None) == capi.E_INVALID
        assert sh._L.bivx_query_sharded_dev_q(sh._h, p(q), vp(dq), vp(dq), 2, 1, 0, C.byref(res), None) == capi.E_INVALID
        assert sh._L.bivx_query_sharded_dev_q(sh._h, None, vp(dq), vp(dq), 2, 1, 0, None, None) == capi.E_INVALID
        assert sh._L.bivx_query_sharded_dev_q(sh._h, None, None, None, 2, 1, 0, C.byref(res), None) == capi.E_INVALID
        # the handle still answers (the failed pointer queries leave no error behind)
        off, hits, rows, _ = sh.query_sharded_device_tensors(dq, dq, batch_order=True)
        assert off.tolist() == [0, 1, 2] and hits.tolist() == [0, 1] and rows is None


@pytest.mark.skipif("__import__('torch').cuda.device_count() < 2", reason="needs two GPUs (the RCCL scatter of the queries)")
def test_two_gpus_equal_the_single_index():
    d = _genome(300_000, 200_000, 11)
    qc, qlo, qhi = d["qchrom"], d["qlow"], d["qhigh"]
    with _built(0, d) as one, _built([0, 1], d) as sh:
        exp = _single(one, qlo, qhi, qc, True)
        off, hits, rows, used_rccl = _dev_q(sh, qlo, qhi, qc, True, True)
        assert used_rccl
        _assert_same((off, hits), exp)
        host = sh.query_sharded_device(qlo, qhi, qc, sort_by_id=True)
        dev = _dev_q(sh, qlo, qhi, qc, True, False)
        _assert_same(dev[:2], host)


def test_c_program(tmp_path):
    exe = str(tmp_path / "sharded_device_queries")
    libdir = os.path.join(ROOT, "binary_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "c", "sharded_device_queries.c"), "-o", exe,
                    "-L", libdir, "-lbivx", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sharded_device_queries: ok" in r.stdout, r.stdout + r.stderr
