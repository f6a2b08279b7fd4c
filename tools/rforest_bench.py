#!/usr/bin/env python3
"""Times the random forest (eegfx_rforest_train, csrc/rforest.hip) on device-resident features.

  python3 tools/rforest_bench.py [--rows N] [--features D] [--rounds R] [--trees T]
                                 [--max-depth K] [--partitions P]

Gaussian features with labels from a noisy linear rule, RandomForestClassifier.java's defaults
(Gini, depth 5, 32 bins, 100 trees, "auto": 7 of 48 features a node, seed 12345).  After one
warm-up call, R timed calls: `train_ms` is the median wall time of a whole call (sample copy,
thresholds, binning, the bag on the host and its upload, every group's histograms / selection /
routing), `hist_ms` the median per histogram launch between HIP events on the context stream
(eegfx_ctx_set_timing), `hist_level_ms` the same summed over a call and divided by the levels that
have a node to split (with these parameters a group is a level of all trees), `bag_ms` the host's
Poisson draws alone (eegfx_poisson_bag, on `bag_threads` threads: the slices, at most the
processors the process may run on), `predict_ms` eegfx_rforest_predict over the same rows.  One
JSON line; a run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--partitions", type=int, default=16)
    args = ap.parse_args()
    import torch

    import eeg_dataanalysispackage_amd as fx
    if not torch.cuda.is_available():
        raise SystemExit("rforest_bench needs a GPU")
    n, d = args.rows, args.features
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, d), dtype=torch.float64, device="cuda", generator=gen)
    w = torch.randn(d, dtype=torch.float64, device="cuda", generator=gen)
    noise = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    y = (X @ w + 0.5 * d ** 0.5 * noise > 0).to(torch.float64)
    ctx = fx.Context(0)
    kw = dict(max_depth=args.max_depth, num_trees=args.trees, num_partitions=args.partitions)
    nodes, off = fx.rforest_train(ctx, X, y, **kw)  # warm-up: allocations
    train_ms, hist_ms, hist_call_ms, predict_ms, bag_ms, launches = [], [], [], [], [], 0
    for _ in range(args.rounds):
        ctx.set_timing(True)  # restarts the event list
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nodes, off = fx.rforest_train(ctx, X, y, **kw)
        train_ms.append((time.perf_counter() - t0) * 1e3)
        launches, ms, _ = ctx.kernel_stats()
        hist_ms.append(ms / launches)
        hist_call_ms.append(ms)
        ctx.set_timing(False)
        t0 = time.perf_counter()
        fx.rforest_predict(ctx, X, nodes, off)
        ctx.synchronize()
        predict_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        fx.poisson_bag(n, args.trees, args.partitions, 12345)
        bag_ms.append((time.perf_counter() - t0) * 1e3)
    # the levels with a node that gets a histogram: the roots, and every node that is not a leaf
    # when it is made
    level = np.floor(np.log2(nodes["id"])).astype(int)
    levels = len(set(level[(level < args.max_depth) & ((nodes["impurity"] != 0.0) | (level == 0))]))
    print(json.dumps({
        "rows": n, "features": d, "trees": args.trees, "max_depth": args.max_depth,
        "partitions": args.partitions, "nodes": int(len(nodes)),
        "train_ms": round(statistics.median(train_ms), 3),
        "train_ms_spread": round((max(train_ms) - min(train_ms)) / statistics.median(train_ms), 3),
        "hist_launches": launches, "hist_ms": round(statistics.median(hist_ms), 4),
        "hist_levels": levels,
        "hist_level_ms": round(statistics.median(hist_call_ms) / max(levels, 1), 4),
        "bag_ms": round(statistics.median(bag_ms), 3),
        "bag_threads": min(args.partitions, 64, len(os.sched_getaffinity(0))),
        "predict_ms": round(statistics.median(predict_ms), 3)}))
    ctx.close()


if __name__ == "__main__":
    main()
