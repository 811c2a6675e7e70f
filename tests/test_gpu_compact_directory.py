"""The compact bucket directory (common.h, dirc_entry: eight entries per 8-byte group, escaped groups read the table) that
k_query_pipe probes instead of the u32 table: decoded on the device entry for entry against the table, and the pipelined
kernel's CSR against the table-probing route (BIVX_PIPE=0) on indexes whose groups escape."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_dirc(idx):
    """(escaped groups, groups) of the built index; every entry must decode to its table word"""
    from binary_amd import capi
    fn = idx._L.bivx_test_check_dirc
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    out = (C.c_uint64 * 3)()
    capi.check(fn(idx._h, out))
    assert out[0] == 0, f"{out[0]} directory entries decode wrongly"
    return int(out[1]), int(out[2])


def _uniform_plus_hotspot(n, hot, seed=0):
    """24 chromosomes of uniform intervals, plus `hot` intervals of chromosome 0 starting inside 40 bp (one cell) at one
    of ten sites (a crowded cell escapes its group unless it is the group's last: that step is the next group's base)"""
    from binary_amd import synth
    d = synth.gen_genome(n, 0, 1000)
    rng = np.random.default_rng(seed + 1)
    lo = (1_000_000 + 1_234_567 * rng.integers(0, 10, hot) + rng.integers(0, 40, hot)).astype(np.uint32)
    hi = (lo + rng.integers(0, 800, hot)).astype(np.uint32)
    return (np.concatenate([d["low"], lo]), np.concatenate([d["high"], hi]),
            np.concatenate([d["chrom"], np.zeros(hot, np.uint32)]))


@pytest.mark.parametrize("spc", [None, "4"])
def test_decodes_to_the_table_config3_like(spc):
    from binary_amd import IntervalIndex, synth
    d = synth.gen_genome(600_000, 0, 1000)
    with _env(**({"BIVX_SLOTS_PER_CELL": spc} if spc else {})), IntervalIndex(0) as idx:
        idx.insert_node(d["low"], d["high"], d["chrom"])
        idx.build()
        esc, groups = _check_dirc(idx)
        assert groups > 0
        if spc is None:
            assert esc * 1000 <= groups  # uniform data at the default density: escapes are rare


def test_decodes_to_the_table_config2_like():
    from binary_amd import IntervalIndex, synth
    L = int(synth.HG38_LENGTHS[0])
    low, high = synth.gen_intervals(300_000, L, 1000, 0)
    with IntervalIndex(0) as idx:
        idx.insert_node(low, high)
        idx.build()
        _check_dirc(idx)


def test_hotspot_groups_escape_and_decode():
    from binary_amd import IntervalIndex
    low, high, chrom = _uniform_plus_hotspot(200_000, 5000)
    with IntervalIndex(0) as idx:
        idx.insert_node(low, high, chrom)
        idx.build()
        esc, _ = _check_dirc(idx)
        assert esc >= 1  # > 15 slots in one cell


def test_segment_boundaries_inside_groups():
    """many small segments (37 chromosomes of 1-40 intervals, two length classes each): table offsets that are not
    multiples of eight, boundaries in the middle of groups"""
    from binary_amd import IntervalIndex
    rng = np.random.default_rng(3)
    lo, hi, ch = [], [], []
    for c in range(37):
        k = int(rng.integers(1, 41))
        l = rng.integers(0, 5_000_000, k).astype(np.uint32)
        ln = np.where(rng.random(k) < 0.3, rng.integers(50_000, 200_000, k), rng.integers(0, 500, k)).astype(np.uint32)
        lo.append(l)
        hi.append(l + ln)
        ch.append(np.full(k, c, np.uint32))
    with IntervalIndex(0) as idx:
        idx.insert_node(np.concatenate(lo), np.concatenate(hi), np.concatenate(ch))
        idx.build()
        assert idx.stats()["n_segments"] >= 37
        _check_dirc(idx)


def _pipe_vs_table(idx, qlo, qhi, qc):
    """CSR of k_query_pipe (compact directory) and of the table-probing route, same buffers"""
    import torch
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    tlo, thi, tc = to(qlo), to(qhi), to(qc)
    q = tlo.numel()
    H = int(idx.count_overlaps_device(tlo, thi, tc)[-1].item())
    out = []
    for mode in (2, 0):
        with _env(BIVX_PIPE=mode):
            if mode == 2:
                assert idx.query_kernel_name(q, H) == "k_query_pipe"
            off = torch.full((q + 1,), -1, dtype=torch.int64, device=dev)
            hits = torch.full((max(H, 1),), -1, dtype=torch.int32, device=dev)
            idx.query_device(tlo, thi, off, hits, qchrom=tc)
            idx.stream_status()
            out.append((off.cpu().numpy(), hits.cpu().numpy()))
    (o2, h2), (o0, h0) = out
    assert np.array_equal(o2, o0) and np.array_equal(h2[:H], h0[:H])
    return H


def test_pipe_csr_equals_the_table_route_on_a_hotspot_index():
    from binary_amd import IntervalIndex, synth
    low, high, chrom = _uniform_plus_hotspot(400_000, 3000)
    g = synth.gen_genome(1000, 200_000, 1000)
    rng = np.random.default_rng(7)
    hq = 100  # queries over the hotspot: windows through escaped groups (few: k_query_pipe wants <= 6 ids per query)
    hlo = (999_000 + 1_234_567 * rng.integers(0, 10, hq) + rng.integers(0, 3000, hq)).astype(np.uint32)
    qlo = np.concatenate([g["qlow"], hlo])
    qhi = np.concatenate([g["qhigh"], hlo + rng.integers(0, 100, hq).astype(np.uint32)])
    qc = np.concatenate([g["qchrom"], np.zeros(hq, np.uint32)])
    p = rng.permutation(qlo.size)
    with IntervalIndex(0) as idx:
        idx.insert_node(low, high, chrom)
        idx.build()
        assert _check_dirc(idx)[0] >= 1
        assert _pipe_vs_table(idx, qlo[p], qhi[p], qc[p]) > 0


def test_dirc_follows_the_table_through_appends_rebuilds_and_clear():
    from binary_amd import IntervalIndex, synth
    g = synth.gen_genome(1000, 150_000, 1000)
    with IntervalIndex(0) as idx:
        d = synth.gen_genome(100_000, 0, 1000)
        idx.insert_node(d["low"], d["high"], d["chrom"])
        idx.build()
        _check_dirc(idx)
        _pipe_vs_table(idx, g["qlow"], g["qhigh"], g["qchrom"])
        low, high, chrom = _uniform_plus_hotspot(300_000, 2000, 2)  # more of everything, and a hotspot
        idx.insert_node(low, high, chrom)
        idx.build()
        assert _check_dirc(idx)[0] >= 1
        _pipe_vs_table(idx, g["qlow"], g["qhigh"], g["qchrom"])
        idx.clear()                                                 # smaller again: the grow-only blocks stay
        d = synth.gen_genome(50_000, 0, 1000)
        idx.insert_node(d["low"], d["high"], d["chrom"])
        idx.build()
        _check_dirc(idx)
        _pipe_vs_table(idx, g["qlow"], g["qhigh"], g["qchrom"])
