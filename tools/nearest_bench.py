#!/usr/bin/env python3
"""Nearest-interval queries at config 3 (24 hg38 chromosomes, 10 M intervals x 10 M range queries; binary_amd/synth.py),
in generation order and position-sorted. Per batch (median over --reps calls, CUDA events around each call):
  - bivx_nearest_dev, unbounded and with max_dist = 1000
  - bivx_any_dev on the same batch (the yardstick: one overlap probe per query)
  - what a caller does without it: widen the queries, find_overlaps_device, reduce (d, id) per query on the device,
    and widen again (x8) for the queries that came back empty, until none is left
Prints one JSON line. Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/nearest_bench.py`
(k_nearest / k_query rows of the stats file)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from binary_amd import IntervalIndex, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--widen", type=int, default=1000, help="first window of the emulation (bp on each side)")
    a = ap.parse_args()

    g = synth.gen_genome(a.intervals, a.queries, 1000)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)
    idx = IntervalIndex(0)
    idx.insert_node(g["low"], g["high"], g["chrom"])
    idx.build()
    ilow = t(g["low"]).to(torch.int64) & 0xFFFFFFFF
    ihigh = t(g["high"]).to(torch.int64) & 0xFFFFFFFF

    def timed(fn):
        ms = []
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), out

    def emulate(dq, dqh, dqc):
        q = dq.numel()
        lo, hi = dq.to(torch.int64) & 0xFFFFFFFF, dqh.to(torch.int64) & 0xFFFFFFFF
        best = torch.full((q,), -1, dtype=torch.int64, device=dev)  # (d << 32 | id); -1: not answered yet
        todo = torch.arange(q, device=dev)
        w, rounds = a.widen, 0
        while todo.numel():
            rounds += 1
            ql, qh = lo[todo], hi[todo]
            wl = (ql - w).clamp(min=0).to(torch.int32)
            wh = (qh + w).clamp(max=0xFFFFFFFF).to(torch.int32)
            off, hits = idx.find_overlaps_device(wl.contiguous(), wh.contiguous(), dqc[todo].contiguous())
            cnt = off[1:] - off[:-1]
            row = torch.repeat_interleave(torch.arange(todo.numel(), device=dev), cnt)
            hid = hits.to(torch.int64) & 0xFFFFFFFF
            d = torch.maximum(torch.maximum(ql[row] - ihigh[hid], ilow[hid] - qh[row]), torch.zeros_like(hid))
            key = torch.full((todo.numel(),), 2**63 - 1, dtype=torch.int64, device=dev)
            key.scatter_reduce_(0, row, d * 2**32 + hid, reduce="amin")
            found = cnt > 0
            best[todo[found]] = key[found]
            todo = todo[~found]
            w *= 8
            if w > 2**33:
                break
        return best, rounds

    out = {"workload": f"config3: {a.intervals} intervals x {a.queries} range queries, 24 hg38 chromosomes", "batches": {}}
    for order in ("generation", "position_sorted"):
        qc, qlo, qhi = g["qchrom"], g["qlow"], g["qhigh"]
        if order == "position_sorted":
            p = np.lexsort((qlo, qc))
            qc, qlo, qhi = qc[p], qlo[p], qhi[p]
        dq, dqh, dqc = t(qlo), t(qhi), t(qc)
        torch.cuda.synchronize()
        ids = torch.empty(a.queries, dtype=torch.int32, device=dev)
        dists = torch.empty_like(ids)
        res = {}
        res["nearest_dev_ms"], _ = timed(lambda: idx.nearest_device(dq, dqh, dqc, ids=ids, dists=dists))
        nid = ids.clone()
        nd = dists.clone()
        res["nearest_dev_max1000_ms"], _ = timed(lambda: idx.nearest_device(dq, dqh, dqc, max_dist=1000, ids=ids,
                                                                             dists=dists))
        res["any_dev_ms"], _ = timed(lambda: idx.find_overlap_device(dq, dqh, dqc))
        ms, (best, rounds) = timed(lambda: emulate(dq, dqh, dqc))
        res["emulation_ms"], res["emulation_rounds"] = ms, rounds
        # the emulation is exact too: it is the check that both answered the same
        eid = (best & 0xFFFFFFFF).to(torch.int64)
        res["emulation_equal"] = bool(torch.equal(eid, nid.to(torch.int64) & 0xFFFFFFFF) and
                                      torch.equal(best >> 32, nd.to(torch.int64) & 0xFFFFFFFF))
        res["nearest_over_any"] = res["nearest_dev_ms"] / res["any_dev_ms"]
        res["emulation_over_nearest"] = res["emulation_ms"] / res["nearest_dev_ms"]
        out["batches"][order] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}
        print(f"{order}: {out['batches'][order]}", file=sys.stderr)
    idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
