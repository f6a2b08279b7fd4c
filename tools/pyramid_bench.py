#!/usr/bin/env python3
"""Times the full-pyramid feature kernel (pyramid.hip, feature sizes above 16) on device-resident
data and answers one question: is the raw -> rows entry faster than the two passes called apart?

  python3 tools/pyramid_bench.py [--epochs N] [--channels C] [--sizes 32,512] [--rounds R]
                                 [--steps K] [--warmup W]

Per feature size, three steps on the same synthetic int16 recording (eegfx_synth_recording,
markers 1000 frames apart):
  from_epochs  eegfx_extract_features_f64 on the materialised epochs (pyramid_from_epochs_kernel)
  fused        eegfx_process_recording_fe on the recording in one call (it runs the two passes
               itself since the fused kernel measured in DESIGN.md 5.4.1 lost at size 512; the
               step stays so that a fused kernel is judged by the same tool)
  two_pass     eegfx_cut_epochs_f64, then eegfx_extract_features_f64 on its rows
Each round times K back-to-back calls of each step between two events on the context's stream,
the steps alternating within a round, after W warm-up calls of every step; the figure of a step is
the median over the rounds and its spread the (max - min) / median of the rounds.  Rates are over
the algorithmic bytes per epoch -- from_epochs: 8 C 512 read + 8 C nf written; fused and two_pass:
the 512 window frames, C float baselines, the position and 8 C nf written (two_pass moves more:
that is its cost) -- as a fraction of the 8 TB/s HBM peak.  `fused_wins` holds when the two-pass
median exceeds the fused median by more than the larger of the two spreads.  One JSON line per
step and one per decision; a run without a GPU fails.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=250_000)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--sizes", default="32,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import eeg_dataanalysispackage_amd as fx
    if not torch.cuda.is_available():
        raise SystemExit("pyramid_bench needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = fx.Context(0, numerics="exact")
    ctx.set_stream(stream.cuda_stream)
    n, C = args.epochs, args.channels
    cols, res = list(range(C)), [0.1] * C
    raw = torch.empty((1000 * n + 2000, C), dtype=torch.int16, device=dev)
    ctx.synth_recording(raw, C, 7)
    pos = torch.arange(1000, 1000 * (n + 1), 1000, dtype=torch.int64, device=dev)
    ep = ctx.cut_epochs(raw, C, cols, res, pos)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / args.steps

    for nf in [int(s) for s in args.sizes.split(",")]:
        feats = torch.empty((n, C * nf), dtype=torch.float64, device=dev)
        steps = {
            "from_epochs": lambda: ctx.extract_features(ep, feature_size=nf, out=feats),
            "fused": lambda: ctx.process_recording(raw, C, cols, res, pos, out=feats,
                                                   feature_size=nf),
            "two_pass": lambda: (ctx.cut_epochs(raw, C, cols, res, pos, out=ep),
                                 ctx.extract_features(ep, feature_size=nf, out=feats)),
        }
        bytes_per_epoch = {
            "from_epochs": 8 * C * 512 + 8 * C * nf,
            "fused": 512 * C * 2 + 4 * C + 8 + 8 * C * nf,
            "two_pass": 512 * C * 2 + 4 * C + 8 + 8 * C * nf,
        }
        sha = {}
        for name, fn in steps.items():
            for _ in range(args.warmup):
                fn()
            ctx.synchronize()
            sha[name] = hashlib.sha256(feats.cpu().numpy().tobytes()).hexdigest()[:16]
        ms = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, fn in steps.items():
                ms[name].append(timed(fn))
        med, spread = {}, {}
        for name in steps:
            med[name] = statistics.median(ms[name])
            spread[name] = (max(ms[name]) - min(ms[name])) / med[name]
            rate = n * bytes_per_epoch[name] / (med[name] * 1e-3)
            print(json.dumps({
                "tool": "pyramid_bench", "step": name, "feature_size": nf, "epochs": n,
                "channels": C, "ms_per_call": round(med[name], 4),
                "rounds_ms": [round(v, 4) for v in ms[name]],
                "spread": round(spread[name], 4),
                "epochs_per_s": round(n / (med[name] * 1e-3), 1),
                "bytes_per_epoch": bytes_per_epoch[name],
                "GBps_algorithmic": round(rate / 1e9, 1),
                "fraction_of_8TBps": round(rate / HBM_PEAK, 4),
                "sha256_16": sha[name]}), flush=True)
        noise = max(spread["fused"], spread["two_pass"])
        gain = (med["two_pass"] - med["fused"]) / med["two_pass"]
        print(json.dumps({
            "tool": "pyramid_bench", "decision": "fused_vs_two_pass", "feature_size": nf,
            "fused_ms": round(med["fused"], 4), "two_pass_ms": round(med["two_pass"], 4),
            "gain": round(gain, 4), "noise": round(noise, 4), "fused_wins": bool(gain > noise),
            "rows_equal": sha["fused"] == sha["two_pass"] == sha["from_epochs"]}), flush=True)
        del feats
    ctx.close()


if __name__ == "__main__":
    main()
