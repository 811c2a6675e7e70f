#!/usr/bin/env python3
"""The gathered call of a sharded handle with host-array queries (bivx_query_sharded_dev: host routing, pageable uploads)
against the same call with device-resident queries (bivx_query_sharded_dev_q: routing kernels on devices[0]), in both of
the latter's modes (rows grouped by device; batch order). Config 3 by default: synth.gen_genome(10 M, 10 M), queries
shuffled, sort_by_id. The three calls alternate, in a rotating order, after a warm-up; each one is timed on the host clock with a device
synchronise inside the window, and the median over --calls calls is reported. Parity is checked on every configuration:
the grouped device-input result must equal the host-input one bit for bit (offsets, ids, rows), and the batch-order
result must be the host-input lists put into batch order. One JSON line per device list (median and min per call).
Kernel times of the routing and permutation kernels: run this under rocprofv3 --kernel-trace --stats, in a run of its own.
usage: tools/sharded_dev_inputs.py [--devices "0;0,0;0,0,0,0"] [--n 10000000] [--q 10000000] [--calls 21] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_order_of(off, hits, rows, q):
    """the grouped CSR (rows answer queries rows[r]) put into batch order with torch: the parity reference"""
    import torch
    dev = off.device
    rows = rows.long()
    length = off[1:] - off[:-1]
    qlen = torch.empty(q, dtype=torch.int64, device=dev)
    qlen[rows] = length
    qoff = torch.zeros(q + 1, dtype=torch.int64, device=dev)
    qoff[1:] = torch.cumsum(qlen, 0)
    src = torch.empty(q, dtype=torch.int64, device=dev)
    src[rows] = off[:-1]
    owner = torch.repeat_interleave(torch.arange(q, device=dev), qlen)
    at = torch.arange(owner.numel(), device=dev) - qoff[owner] + src[owner]
    return qoff, hits[at]


def main():
    import torch
    from binary_amd import IntervalIndex, capi, synth
    from binary_amd.interval_index import _take_sharded_result
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--devices", default="0;0,0;0,0,0,0", help="device lists separated by ';'")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--q", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default="", help="recorded in the output")
    a = ap.parse_args()
    d = synth.gen_genome(a.n, a.q)
    perm = np.random.default_rng(0).permutation(d["qlow"].size)
    qc, qlo, qhi = (np.ascontiguousarray(d[k][perm]) for k in ("qchrom", "qlow", "qhigh"))
    q = int(qlo.size)
    to = lambda x: torch.from_numpy(x.view(np.int32)).to("cuda:0")
    d_qc, d_qlo, d_qhi = to(qc), to(qlo), to(qhi)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    t = lambda x: C.c_void_p(x.data_ptr())
    for spec in a.devices.split(";"):
        devices = [int(x) for x in spec.split(",")]
        with IntervalIndex(devices) as sh:
            sh.insert_node(d["low"], d["high"], d["chrom"])
            sh.build()
            L, h = sh._L, sh._h
            res = capi.ShardedResult()
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            calls = {
                "host_input": lambda: L.bivx_query_sharded_dev(h, p(qc), p(qlo), p(qhi), q, 1, C.byref(res)),
                "device_input": lambda: L.bivx_query_sharded_dev_q(h, t(d_qc), t(d_qlo), t(d_qhi), q, 1, 0, C.byref(res), stream),
                "device_input_batch_order": lambda: L.bivx_query_sharded_dev_q(h, t(d_qc), t(d_qlo), t(d_qhi), q, 1, 1,
                                                                               C.byref(res), stream),
            }
            # parity, on this configuration
            capi.check(calls["host_input"]())
            h_off, h_hits, h_rows, _ = _take_sharded_result(res)
            capi.check(calls["device_input"]())
            g_off, g_hits, g_rows, _ = _take_sharded_result(res)
            capi.check(calls["device_input_batch_order"]())
            b_off, b_hits, b_rows, _ = _take_sharded_result(res)
            e_off, e_hits = batch_order_of(h_off, h_hits, h_rows, q)
            parity = bool(torch.equal(h_off, g_off) and torch.equal(h_hits, g_hits) and torch.equal(h_rows, g_rows)
                          and b_rows is None and torch.equal(b_off, e_off) and torch.equal(b_hits, e_hits))
            del h_off, h_hits, h_rows, g_off, g_hits, g_rows, b_off, b_hits, e_off, e_hits
            for _ in range(a.warmup):
                for f in calls.values():
                    capi.check(f())
            times = {k: [] for k in calls}
            names = list(calls)
            for i in range(a.calls):
                # alternating, in a rotating order: the three share whatever the machine does meanwhile, and no call always
                # comes right after the host-input one (which leaves the GPU idle for tens of ms)
                for k in names[i % 3:] + names[:i % 3]:
                    f = calls[k]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    capi.check(f())
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            out = {"devices": devices, "queries": q, "intervals": int(d["low"].size), "hits": int(res.total),
                   "calls": a.calls, "parity": parity, "commit": a.commit}
            out.update({f"{k}_median_ms": round(statistics.median(v), 3) for k, v in times.items()})
            out.update({f"{k}_min_ms": round(min(v), 3) for k, v in times.items()})
            print(json.dumps(out), flush=True)
            if not parity:
                sys.exit(1)


if __name__ == "__main__":
    main()
