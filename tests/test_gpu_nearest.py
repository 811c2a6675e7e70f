"""bivx_nearest / bivx_nearest_dev (binary_amd/csrc/nearest.hip): per query the stored interval of smallest
(max(0, q.low - high, low - q.high), id) on the query's chromosome, within max_dist. Checked against a hand-checked
fixture, a numpy brute force on randomised data with edge cases, bivx_any (max_dist = 0), the verified overlap path at
config 3 size, the device entry point, sharded handles, the error paths and the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 0xFFFFFFFF
NO_HIT = 0xFFFFFFFF


def _brute(chrom, low, high, qc, qlo, qhi, max_dist=U32, typ=None, svtype=0):
    """(ids, dists) by exhaustion: per chromosome, argmin over (d, id) of d = max(0, q.low - high, low - q.high)."""
    q = qlo.size
    ids = np.full(q, NO_HIT, np.uint32)
    dists = np.full(q, U32, np.uint32)
    sel = np.ones(low.size, bool) if not svtype else (typ == svtype)
    for c in np.unique(qc):
        iv = np.nonzero(sel & (chrom == c))[0]
        qs = np.nonzero(qc == c)[0]
        if iv.size == 0:
            continue
        il, ih = low[iv].astype(np.int64), high[iv].astype(np.int64)
        step = max(1, 4_000_000 // iv.size)
        for s in range(0, qs.size, step):
            qq = qs[s:s + step]
            ql, qh = qlo[qq].astype(np.int64)[:, None], qhi[qq].astype(np.int64)[:, None]
            d = np.maximum(np.maximum(ql - ih[None, :], il[None, :] - qh), 0)
            bd = d.min(axis=1)  # (d up to 2^32 - 1: a packed (d << 32 | id) key would not fit an int64)
            bi = np.where(d == bd[:, None], iv[None, :], np.iinfo(np.int64).max).min(axis=1)
            ok = bd <= max_dist
            ids[qq[ok]] = bi[ok].astype(np.uint32)
            dists[qq[ok]] = bd[ok].astype(np.uint32)
    return ids, dists


def _edge_dataset(seed=3):
    """several chromosomes (1 and 4 empty), length classes 50 bp .. 100 kbp, duplicates, a positional hotspot (windows
    beyond the wavefront's trim), low > high intervals, coordinates 0 and 2^32 - 1, and svtypes 1..3."""
    rng = np.random.default_rng(seed)
    parts = []
    # chromosome 0: the k_query_pipe_ms shape, log-uniform lengths over many classes
    n0 = 12_000
    lo = rng.integers(0, 50_000_000, n0)
    parts.append((0, lo, lo + np.exp(rng.uniform(np.log(50), np.log(100_000), n0)).astype(np.int64)))
    # chromosome 2: short intervals, duplicates and a hotspot of 3000 intervals starting at one position
    n2 = 8_000
    lo = rng.integers(1_000, 5_000_000, n2)
    hi = lo + rng.integers(0, 1000, n2)
    lo[::5], hi[::5] = lo[1::5][: lo[::5].size], hi[1::5][: hi[::5].size]
    hot = np.full(3000, 2_500_000)
    parts.append((2, np.concatenate([lo, hot]), np.concatenate([hi, hot + rng.integers(0, 3000, 3000)])))
    # chromosome 3: sparse, with the coordinate extremes and inverted intervals
    lo = np.concatenate([rng.integers(0, U32, 300), [0, 0, U32, U32 - 5, 100]])
    hi = np.concatenate([np.minimum(lo[:300] + rng.integers(0, 10_000, 300), U32), [0, 7, U32, U32, 90]])
    inv = rng.random(300) < 0.1
    hi[:300][inv] = lo[:300][inv] - np.minimum(lo[:300][inv], rng.integers(1, 500, inv.sum()))
    parts.append((3, lo, hi))
    chrom = np.concatenate([np.full(p[1].size, p[0], np.uint32) for p in parts])
    low = np.concatenate([p[1] for p in parts]).astype(np.uint32)
    high = np.concatenate([p[2] for p in parts]).astype(np.uint32)
    perm = rng.permutation(low.size)  # append order unrelated to position
    chrom, low, high = chrom[perm], low[perm], high[perm]
    typ = rng.integers(1, 4, low.size).astype(np.uint8)
    # queries: chromosomes 0..5 (1 and 4 empty, 5 beyond every id), near and far, inverted, at the extremes
    q = 20_000
    qc = rng.integers(0, 6, q).astype(np.uint32)
    qlo = rng.integers(0, 60_000_000, q)
    qlo[::7] = rng.integers(0, U32, qlo[::7].size)                 # far outside every interval
    qhi = qlo + rng.integers(0, 5000, q)
    qhi[::11] = qlo[::11] - np.minimum(qlo[::11], rng.integers(1, 2000, qhi[::11].size))  # low > high queries
    qlo[::13], qhi[::13] = 0, 0
    qlo[::17], qhi[::17] = U32, U32
    qlo[5::19], qhi[5::19] = 2_500_100, 2_500_200                    # in the hotspot
    qc[5::19] = 2
    qhi = np.minimum(qhi, U32)
    return chrom, low, high, typ, qc, qlo.astype(np.uint32), qhi.astype(np.uint32)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _built(chrom, low, high, typ=None, full_sort=False, device=0):
    from binary_amd import IntervalIndex
    idx = IntervalIndex(device)
    idx.insert_node(low, high, chrom, svtype=typ)
    with _env(BIVX_BUILD_FULL_SORT="1" if full_sort else None):
        idx.build()
    return idx


def test_reference_fixture_by_hand():
    low = np.array([16, 8, 5, 0, 6, 15, 25, 17, 19, 26], np.uint32)
    high = np.array([21, 9, 8, 3, 10, 23, 30, 19, 20, 26], np.uint32)
    cases = [((11, 13), U32, 4, 1), ((12, 13), U32, 4, 2), ((24, 24), U32, 5, 1), ((40, 50), U32, 6, 10),
             ((40, 50), 9, NO_HIT, None), ((7, 7), U32, 2, 0)]
    with _built(np.zeros(10, np.uint32), low, high) as idx:
        for (ql, qh), md, eid, ed in cases:
            ids, d = idx.nearest([ql], [qh], max_dist=None if md == U32 else md)
            assert int(ids[0]) == eid, ((ql, qh), md, ids, d)
            if ed is not None:
                assert int(d[0]) == ed


@pytest.mark.parametrize("full_sort", [False, True])
def test_random_parity_with_brute_force(full_sort):
    chrom, low, high, typ, qc, qlo, qhi = _edge_dataset()
    with _built(chrom, low, high, typ, full_sort) as idx:
        for md in (0, 1, 1000, U32):
            ids, d = idx.nearest(qlo, qhi, qc, max_dist=md)
            eids, ed = _brute(chrom, low, high, qc, qlo, qhi, md)
            bad = np.nonzero(ids != eids)[0]
            assert bad.size == 0, (md, bad[:5], ids[bad[:5]], eids[bad[:5]], d[bad[:5]], ed[bad[:5]])
            hit = eids != NO_HIT
            assert np.array_equal(d[hit], ed[hit]) and np.all(d[~hit] == U32)
        # one svtype of a typed index; a type the index does not hold
        for t in (2, 9):
            ids, d = idx.nearest(qlo, qhi, qc, max_dist=100_000, svtype=t)
            eids, ed = _brute(chrom, low, high, qc, qlo, qhi, 100_000, typ, t)
            assert np.array_equal(ids, eids) and np.array_equal(d[eids != NO_HIT], ed[eids != NO_HIT])
        assert np.all(idx.nearest(qlo[:100], qhi[:100], qc[:100], svtype=9)[0] == NO_HIT)
        # dist_out == NULL, on the mailbox path and the uploaded one
        L = idx._L
        for q in (40, 5000):
            out = np.empty(q, np.uint32)
            from binary_amd import capi
            capi.check(L.bivx_nearest(idx._h, qc[:q].ctypes.data, qlo[:q].ctypes.data, qhi[:q].ctypes.data, q, U32, 0,
                                      out.ctypes.data, None))
            assert np.array_equal(out, _brute(chrom, low, high, qc[:q], qlo[:q], qhi[:q])[0])


def test_max_dist_zero_is_bivx_any_config2():
    from binary_amd import synth
    G = int(synth.HG38_LENGTHS[0])
    low, high = synth.gen_intervals(1_000_000, G)
    qlo, qhi = synth.gen_point_queries(1_000_000, G)
    with _built(None, low, high) as idx:
        ids, d = idx.nearest(qlo, qhi, max_dist=0)
        first = idx.find_overlap(qlo, qhi)
        assert np.array_equal(ids, first)
        assert np.all(d[ids != NO_HIT] == 0)


def test_device_entry_point_equals_host_on_any_stream():
    import torch
    chrom, low, high, typ, qc, qlo, qhi = _edge_dataset(seed=8)
    with _built(chrom, low, high, typ) as idx:
        ids, d = idx.nearest(qlo, qhi, qc, max_dist=5000)
        t = lambda a: torch.from_numpy(a.view(np.int32)).to("cuda:0")
        dq, dqh, dqc = t(qlo), t(qhi), t(qc)
        torch.cuda.synchronize()
        for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
            with torch.cuda.stream(stream):
                di, dd = idx.nearest_device(dq, dqh, dqc, max_dist=5000)
            stream.synchronize()
            assert np.array_equal(di.cpu().numpy().view(np.uint32), ids)
            assert np.array_equal(dd.cpu().numpy().view(np.uint32), d)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_sharded_handles_equal_single_device(devices):
    from binary_amd import IntervalIndex, capi
    chrom, low, high, typ, qc, qlo, qhi = _edge_dataset(seed=5)
    for by_chrom in (True, False):
        c = chrom if by_chrom else np.zeros_like(chrom)
        cq = qc if by_chrom else np.zeros_like(qc)
        with _built(c, low, high, typ) as one, IntervalIndex(devices) as sh:
            sh.insert_node(low, high, c, svtype=typ)
            sh.build()
            for md, t in ((U32, 0), (1000, 0), (U32, 3)):
                a = one.nearest(qlo, qhi, cq, max_dist=md, svtype=t)
                b = sh.nearest(qlo, qhi, cq, max_dist=md, svtype=t)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (devices, by_chrom, md, t)
            out = np.empty(4, np.uint32)
            rc = sh._L.bivx_nearest_dev(sh._h, None, qlo.ctypes.data, qhi.ctypes.data, 4, U32, 0, out.ctypes.data, None,
                                        None)
            assert rc == capi.E_STATE


def test_errors():
    from binary_amd import IntervalIndex, capi
    lo = np.array([5, 9], np.uint32)
    out = np.empty(2, np.uint32)
    with IntervalIndex(0) as idx:
        L = idx._L
        idx.insert_node(lo, lo + 1)
        assert L.bivx_nearest(idx._h, None, lo.ctypes.data, lo.ctypes.data, 2, U32, 0, out.ctypes.data, None) == capi.E_STATE
        assert L.bivx_nearest_dev(idx._h, None, None, None, 0, U32, 0, None, None, None) == capi.E_STATE
        idx.build()
        assert L.bivx_nearest(idx._h, None, lo.ctypes.data, lo.ctypes.data, 2, U32, 0, None, None) == capi.E_INVALID
        assert L.bivx_nearest(idx._h, None, None, lo.ctypes.data, 2, U32, 0, out.ctypes.data, None) == capi.E_INVALID
        assert L.bivx_nearest_dev(idx._h, None, None, None, 2, U32, 0, None, None, None) == capi.E_INVALID
        assert L.bivx_nearest(idx._h, None, None, None, 0, U32, 0, None, None) == 0
        assert L.bivx_nearest_dev(idx._h, None, None, None, 0, U32, 0, None, None, None) == 0
        ids, d = idx.nearest(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        assert ids.size == 0 and d.size == 0
    with IntervalIndex([0, 0]) as sh:
        sh.insert_node(lo, lo + 1)
        assert sh._L.bivx_nearest(sh._h, None, lo.ctypes.data, lo.ctypes.data, 2, U32, 0, out.ctypes.data,
                                  None) == capi.E_STATE


@pytest.mark.parametrize("position_sorted", [False, True])
def test_config3_full_size_against_the_overlap_path(position_sorted):
    """10 M intervals x 10 M range queries (bench.py config 3), checked on the device with bivx_any_dev: the distance is
    the one recomputed from the answer's coordinates, nothing lies closer (the query widened by d - 1 meets nothing) and
    the answer is the smallest id at that distance (the query widened by d meets it first)."""
    import torch
    from binary_amd import synth
    g = synth.gen_genome(10_000_000, 10_000_000, 1000)
    qc, qlo, qhi = g["qchrom"], g["qlow"], g["qhigh"]
    if position_sorted:
        p = np.lexsort((qlo, qc))
        qc, qlo, qhi = qc[p], qlo[p], qhi[p]
    with _built(g["chrom"], g["low"], g["high"]) as idx:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
        dq, dqh, dqc = t(qlo), t(qhi), t(qc)
        di, dd = idx.nearest_device(dq, dqh, dqc)
        ids = di.cpu().numpy().view(np.uint32)
        d = dd.cpu().numpy().view(np.uint32)
        assert np.all(ids != NO_HIT)  # every chromosome holds intervals
        c, lo, hi = idx.get_intervals(ids)
        assert np.array_equal(c, qc)
        exp = np.maximum(np.maximum(qlo.astype(np.int64) - hi, lo.astype(np.int64) - qhi), 0)
        assert np.array_equal(d.astype(np.int64), exp)
        d64 = d.astype(np.int64)

        def widened(by):
            wl = np.maximum(qlo.astype(np.int64) - by, 0).astype(np.uint32)
            wh = np.minimum(qhi.astype(np.int64) + by, U32).astype(np.uint32)
            return idx.find_overlap_device(t(wl), t(wh), dqc).cpu().numpy().view(np.uint32)

        closer = widened(np.maximum(d64 - 1, 0))
        assert np.all(closer[d64 > 0] == NO_HIT)
        assert np.array_equal(widened(d64), ids)


def test_cpp_facade_find_nearest(tmp_path):
    from binary_amd import _build
    _build.build_lib()
    exe = str(tmp_path / "facade_nearest")
    libdir = os.path.join(ROOT, "binary_amd")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_nearest.cpp"), "-o", exe, "-L", libdir, "-lbivx",
                    "-pthread", f"-Wl,-rpath,{libdir}"], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
