#!/usr/bin/env python3
"""Times the float32 epoch entries beside the float64 entries they mirror, on device-resident
data, and writes one JSON line per leg under profiles/epochs_f32/.

  python3 tools/epochs_f32_bench.py [--epochs N] [--channels C] [--rounds R] [--steps K]
                                    [--warmup W] [--host-epochs H] [--f64-only] [--out NAME]

Legs, on one synthetic int16 recording (eegfx_synth_recording, markers 1000 frames apart):
  cut            eegfx_cut_epochs_f64 / _f32
  one_pass       eegfx_process_recording_epochs / _f32 (epochs + the 16-feature rows)
  extract16      eegfx_extract_features_f64 / _f32 from device epochs, feature size 16, EXACT
  extract16_fma  the same under EEGFX_FMA
  extract512     the same at feature size 512 (EXACT under both settings)
  host           eegfx_extract_features_f64 / _f32 on a host batch of H epochs (default 100k):
                 the chunked copies of the window columns; wall-clock, the call synchronises
  fe_100_16      eegfx_process_recording_fe at (skip 100, size 16): it has no f32 entry; its
                 scratch epochs are float32 (the same leg on an older build runs over doubles)
Device legs: each round times K back-to-back calls between two events on the context's stream,
the legs alternating within a round, after W warm-up calls of every leg; a leg's figure is the
median over the R rounds, with the rounds' min and max beside it.  `predicted_ratio` is the
f64 / f32 ratio of the algorithmic bytes per epoch (the byte model of DESIGN.md), `ratio` the
measured f64 / f32 ratio of the medians.  --f64-only times the f64 legs alone through calls every
build has, for the comparison with the parent commit.  A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)


def bytes_model(C):
    """Algorithmic bytes per epoch of each leg as (f64, f32): the 850 int16 frames an epoch
    spans (100 baseline + 750), the epoch rows written or the window rows read, the rows out."""
    raw, ep64, ep32, win64, win32 = 850 * C * 2, 6000 * C, 3000 * C, 4096 * C, 2048 * C
    f16, f512 = 8 * C * 16, 8 * C * 512
    return {
        "cut": (raw + ep64, raw + ep32),
        "one_pass": (raw + ep64 + f16, raw + ep32 + f16),
        "extract16": (win64 + f16, win32 + f16),
        "extract16_fma": (win64 + f16, win32 + f16),
        "extract512": (win64 + f512, win32 + f512),
        "host": (win64 + f16, win32 + f16),          # bytes over the host link
        "fe_100_16": (raw + ep64 + win64 + f16, raw + ep32 + win32 + f16),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1_000_000)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-epochs", type=int, default=100_000)
    ap.add_argument("--f64-only", action="store_true")
    ap.add_argument("--out", default="epochs_f32_bench.jsonl",
                    help="file name under profiles/epochs_f32/")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "epochs_f32"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eeg_dataanalysispackage_amd as fx
    if not torch.cuda.is_available():
        raise SystemExit("epochs_f32_bench needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = fx.Context(0, numerics="exact")
    fma = fx.Context(0, numerics="fma")
    ctx.set_stream(stream.cuda_stream)
    fma.set_stream(stream.cuda_stream)
    n, C, f32 = args.epochs, args.channels, not args.f64_only
    cols, res = list(range(C)), [0.1] * C
    raw = torch.empty((1000 * n + 2000, C), dtype=torch.int16, device=dev)
    ctx.synth_recording(raw, C, 7)
    pos = torch.arange(1000, 1000 * (n + 1), 1000, dtype=torch.int64, device=dev)
    ep64 = ctx.cut_epochs(raw, C, cols, res, pos)
    ep32 = ctx.cut_epochs(raw, C, cols, res, pos, dtype=np.float32) if f32 else None
    f16 = torch.empty((n, C * 16), dtype=torch.float64, device=dev)
    f512 = torch.empty((n, C * 512), dtype=torch.float64, device=dev)
    h = min(args.host_epochs, n)
    hep64 = ep64[:h].cpu().numpy()
    hep32 = ep32[:h].cpu().numpy() if f32 else None
    hout = np.empty((h, C * 16))

    # leg -> {"f64": fn, "f32": fn}
    legs = {
        "cut": {"f64": lambda: ctx.cut_epochs(raw, C, cols, res, pos, out=ep64)},
        "one_pass": {"f64": lambda: ctx.process_recording_epochs(raw, C, cols, res, pos, out=f16,
                                                                 epochs_out=ep64)},
        "extract16": {"f64": lambda: ctx.extract_features(ep64, out=f16)},
        "extract16_fma": {"f64": lambda: fma.extract_features(ep64, out=f16)},
        "extract512": {"f64": lambda: ctx.extract_features(ep64, feature_size=512, out=f512)},
        "fe_100_16": {"f64": lambda: ctx.process_recording(raw, C, cols, res, pos, out=f16,
                                                           skip=100, feature_size=16)},
    }
    host_legs = {"host": {"f64": lambda: ctx.extract_features(hep64, out=hout)}}
    if f32:
        legs["cut"]["f32"] = lambda: ctx.cut_epochs(raw, C, cols, res, pos, out=ep32,
                                                    dtype=np.float32)
        legs["one_pass"]["f32"] = lambda: ctx.process_recording_epochs(
            raw, C, cols, res, pos, out=f16, epochs_out=ep32, epochs_dtype=np.float32)
        legs["extract16"]["f32"] = lambda: ctx.extract_features_f32(ep32, out=f16)
        legs["extract16_fma"]["f32"] = lambda: fma.extract_features_f32(ep32, out=f16)
        legs["extract512"]["f32"] = lambda: ctx.extract_features_f32(ep32, feature_size=512,
                                                                     out=f512)
        host_legs["host"]["f32"] = lambda: ctx.extract_features_f32(hep32, out=hout)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / args.steps

    def timed_host(fn):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    ms = {}
    for group, timer in ((legs, timed), (host_legs, timed_host)):
        for leg in group.values():
            for fn in leg.values():
                for _ in range(args.warmup):
                    fn()
        ctx.synchronize()
        fma.synchronize()
        for _ in range(args.rounds):
            for name, leg in group.items():
                for kind, fn in leg.items():
                    ms.setdefault((name, kind), []).append(timer(fn))

    model = bytes_model(C)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.out), "w") as f:
        for name in list(legs) + list(host_legs):
            rec = {"tool": "epochs_f32_bench", "leg": name, "channels": C,
                   "epochs": h if name == "host" else n, "steps": args.steps,
                   "timer": "wall" if name == "host" else "events",
                   "bytes_per_epoch_f64": model[name][0], "bytes_per_epoch_f32": model[name][1],
                   "predicted_ratio": round(model[name][0] / model[name][1], 3)}
            for kind in ("f64", "f32"):
                if (name, kind) in ms:
                    v = ms[(name, kind)]
                    rec[kind] = {"median_ms": round(statistics.median(v), 4),
                                 "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                 "rounds_ms": [round(x, 4) for x in v]}
            if "f32" in rec:
                rec["ratio"] = round(rec["f64"]["median_ms"] / rec["f32"]["median_ms"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    ctx.close()
    fma.close()


if __name__ == "__main__":
    main()
