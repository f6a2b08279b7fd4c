#!/usr/bin/env python3
"""Times the decision tree (eegfx_dtree_train, csrc/dtree.hip) on device-resident features.

  python3 tools/dtree_bench.py [--rows N] [--features D] [--rounds R] [--max-depth K]

Gaussian features with labels from a noisy linear rule, Strategy.defaultStrategy's parameters
(Gini, depth 5, 32 bins).  After one warm-up call, R timed calls: `train_ms` is the median wall
time of a whole call (sample copy, thresholds, binning, every level's histogram / selection /
routing), `hist_ms` the median per histogram launch between HIP events on the context stream
(eegfx_ctx_set_timing), and `hist_rate` the n d + 5 n bytes a launch must read (the bins, the slot
and the label of every row) over that time, as a fraction of the 8 TB/s HBM peak.  One JSON line;
a run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-depth", type=int, default=5)
    args = ap.parse_args()
    import torch

    import eeg_dataanalysispackage_amd as fx
    if not torch.cuda.is_available():
        raise SystemExit("dtree_bench needs a GPU")
    n, d = args.rows, args.features
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, d), dtype=torch.float64, device="cuda", generator=gen)
    w = torch.randn(d, dtype=torch.float64, device="cuda", generator=gen)
    noise = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    y = (X @ w + 0.5 * d ** 0.5 * noise > 0).to(torch.float64)
    ctx = fx.Context(0)
    nodes = fx.dtree_train(ctx, X, y, max_depth=args.max_depth)  # warm-up: allocations
    train_ms, hist_ms, launches = [], [], 0
    for _ in range(args.rounds):
        ctx.set_timing(True)  # restarts the event list
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nodes = fx.dtree_train(ctx, X, y, max_depth=args.max_depth)
        train_ms.append((time.perf_counter() - t0) * 1e3)
        launches, ms, _ = ctx.kernel_stats()
        hist_ms.append(ms / launches)
        ctx.set_timing(False)
    h = statistics.median(hist_ms)
    print(json.dumps({
        "rows": n, "features": d, "max_depth": args.max_depth, "nodes": int(len(nodes)),
        "train_ms": round(statistics.median(train_ms), 3),
        "train_ms_spread": round((max(train_ms) - min(train_ms)) / statistics.median(train_ms), 3),
        "hist_launches": launches, "hist_ms": round(h, 4),
        "hist_bytes": n * d + 5 * n,
        "hist_rate_of_hbm_peak": round((n * d + 5 * n) / (h * 1e-3) / HBM_PEAK, 4)}))
    ctx.close()


if __name__ == "__main__":
    main()
