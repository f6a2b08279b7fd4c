#!/usr/bin/env python3
"""Per-iteration time of eegfx_nn_train on device rows, with two
references measured in the same process: the logistic iteration of eegfx_logreg_sgd_train on the
same rows (it reads the same bytes: the floor) and a PyTorch float64 forward + backward of the
same network with torch.autograd (the off-the-shelf route).

    python tools/nn_bench.py [--rows 1000000] [--d 48] [--hidden 16] [--iterations 20] [--out F]

The nn legs come from Context.kernel_stats (HIP events around each iteration's two launches);
the logistic leg, which records no events, from the wall time of a long call minus a short one;
the torch leg from torch.cuda events.  One JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import eeg_dataanalysispackage_amd as fx  # noqa: E402
from eeg_dataanalysispackage_amd import classification as clf  # noqa: E402

HBM_BYTES_PER_S = 8e12


def flops_per_row(d, widths):
    """Multiply-adds of forward, backward and the weight gradients, two flops each."""
    n_in = [d] + list(widths[:-1])
    fwd = sum(i * o for i, o in zip(n_in, widths))
    back = sum(i * o for i, o in zip(n_in[1:], widths[1:]))
    return 2 * (2 * fwd + back)


def nn_leg(ctx, X, y, model, iterations):
    p0 = clf.nn_init_params(model)
    clf.nn_train(ctx, X, y, model, p0, num_iterations=2)  # warm: allocations, code load
    ctx.set_timing(True)
    clf.nn_train(ctx, X, y, model, p0, num_iterations=iterations)
    launches, ms, _ = ctx.kernel_stats()
    ctx.set_timing(False)
    assert launches == iterations
    return ms / iterations


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def logreg_leg(ctx, X, y, iterations):
    run = lambda it: clf.sgd_train(ctx, X, y, num_iterations=it, reg_param=0.01,
                                   convergence_tol=0.0)
    run(2)
    short = min(wall(lambda: run(iterations)) for _ in range(3))
    long = min(wall(lambda: run(6 * iterations)) for _ in range(3))
    return (long - short) / (5 * iterations)


def torch_leg(X, y, model, iterations):
    layers, n_in = [], model.d
    for w in model.widths:
        layers.append(torch.nn.Linear(n_in, w, dtype=torch.float64, device="cuda"))
        n_in = w
    target = torch.stack([y, (1 - y).abs()], dim=1)

    def step():
        a = X
        for i, lin in enumerate(layers):
            a = lin(a)
            a = torch.tanh(a) if i < len(layers) - 1 else torch.log_softmax(a, dim=1)
        loss = -(target * a).sum() / X.shape[0]
        for lin in layers:
            lin.zero_grad(set_to_none=True)
        loss.backward()

    for _ in range(3):
        step()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iterations):
        step()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=48)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(a.rows, a.d, dtype=torch.float64, device="cuda", generator=gen)
    X /= X.norm(dim=1, keepdim=True)
    y = (torch.rand(a.rows, dtype=torch.float64, device="cuda", generator=gen) < 0.5).double()
    widths = (a.hidden, 2)
    row_bytes = 8 * (a.d + 1)
    ctx = fx.Context(0)
    lines = []
    try:
        for updater in ("sgd", "nesterovs"):
            m = clf.NnModel(d=a.d, widths=widths, activations=("tanh", "softmax"),
                            loss="negativeloglikelihood", updater=updater)
            ms = nn_leg(ctx, X, y, m, a.iterations)
            lines.append(dict(leg=f"eegfx_nn_train {updater}", ms_per_iteration=ms,
                              hbm_fraction=a.rows * row_bytes / (ms * 1e-3) / HBM_BYTES_PER_S,
                              fp64_tflops=a.rows * flops_per_row(a.d, widths) / (ms * 1e-3) / 1e12))
        ms = logreg_leg(ctx, X, y, a.iterations)
        lines.append(dict(leg="eegfx_logreg_sgd_train (floor: the same bytes)", ms_per_iteration=ms,
                          hbm_fraction=a.rows * row_bytes / (ms * 1e-3) / HBM_BYTES_PER_S))
        ms = torch_leg(X, y, clf.NnModel(d=a.d, widths=widths, activations=("tanh", "softmax")),
                       a.iterations)
        lines.append(dict(leg="torch float64 autograd forward + backward", ms_per_iteration=ms))
    finally:
        ctx.close()
    head = dict(rows=a.rows, d=a.d, widths=widths, iterations=a.iterations,
                bytes_per_row=row_bytes, flops_per_row=flops_per_row(a.d, widths),
                device=torch.cuda.get_device_name(0))
    text = "\n".join(json.dumps(dict(head, **ln)) for ln in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
