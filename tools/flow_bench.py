#!/usr/bin/env python3
"""Times the train/test flow's data movement on synthetic recordings.

Two figures, recorded with no threshold:

* wall time of OffLineDataProvider.split(device=True) against the route to the same four device
  arrays without it: pipeline.train_test_features (getData to the host, the shuffle and the
  fancy indexing there, the epochs uploaded again for extraction) followed by an upload of the
  four arrays.  --repeat interleaved alternations of the two, median (min - max) of each;
* the gather kernel's achieved bytes per second at d = 48 and d = 1 over the same number of rows
  in shuffled order, from Context.kernel_stats, as a fraction of the 8 TB/s HBM peak.

Writes --files int16 recordings of --frames frames x 3 channels with a marker every --spacing
frames (about files * frames / spacing selected epochs; the epochs overlap, which costs the
kernels nothing) into a temporary directory.

    python tools/flow_bench.py [--files 16] [--frames 6250000] [--spacing 100] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import eeg_dataanalysispackage_amd as fx  # noqa: E402
from eeg_dataanalysispackage_amd import pipeline  # noqa: E402
from odp_multi_bench import write_directory  # noqa: E402

HBM_PEAK = 8e12


def summary(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def host_route(odp, fe, device):
    ftr, ytr, fte, yte = pipeline.train_test_features(odp, fe)
    out = [torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)
           for a in (ftr, ytr, fte, yte)]
    torch.cuda.synchronize()
    return out


def device_route(odp, fe, ctx):
    out = odp.split(fe, device=True, context=ctx)
    ctx.synchronize()
    torch.cuda.synchronize()
    return out


def gather_rate(ctx, n, d, launches):
    src = torch.rand((n, d) if d > 1 else (n,), dtype=torch.float64, device="cuda")
    idx = torch.from_numpy(pipeline.native_shuffle(n)).cuda()
    out = torch.empty_like(src)
    pipeline.gather_rows(ctx, src, idx, out=out)  # warm: buffers, code object
    ctx.set_timing(True)
    for _ in range(launches):
        pipeline.gather_rows(ctx, src, idx, out=out)
    count, ms, nbytes = ctx.kernel_stats()
    ctx.set_timing(False)
    rate = nbytes / (ms * 1e-3)
    return {"d": d, "rows": n, "launches": count, "ms_per_launch": ms / count,
            "bytes_per_launch": nbytes // count, "bytes_per_s": rate,
            "fraction_of_8TBps": rate / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--frames", type=int, default=6_250_000)
    ap.add_argument("--spacing", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args()
    ctx = fx.Context(0)
    fe = fx.WaveletTransform(8, 512, 175, 16, context=ctx)
    result = {"files": a.files, "frames": a.frames, "spacing": a.spacing, "repeat": a.repeat}
    with tempfile.TemporaryDirectory() as root:
        info = write_directory(root, a.files, a.frames, a.spacing)
        odp = fx.OffLineDataProvider([info], context=ctx)
        t0 = time.perf_counter()
        odp.loadData()
        result["load_s"] = time.perf_counter() - t0
        assert odp.last_error == "", odp.last_error
        n = result["epochs"] = odp.num_epochs()
        print(f"{n} epochs loaded in {result['load_s']:.2f} s", flush=True)
        device = f"cuda:{ctx.device}"
        times = {"split_device": [], "train_test_features_upload": []}
        for r in range(a.repeat + 1):  # the first alternation warms buffers and the allocator
            t0 = time.perf_counter()
            dev = device_route(odp, fe, ctx)
            t1 = time.perf_counter()
            host = host_route(odp, fe, device)
            t2 = time.perf_counter()
            if r == 0:  # the same four arrays
                for x, y in zip(dev, host):
                    assert torch.equal(x.view(torch.int64), y.view(torch.int64))
            else:
                times["split_device"].append(t1 - t0)
                times["train_test_features_upload"].append(t2 - t1)
            print(f"alternation {r}: split {t1 - t0:.4f} s, host route {t2 - t1:.3f} s",
                  flush=True)
            del dev, host
        result["legs"] = {k: summary(v) for k, v in times.items()}
        odp.close()
    result["gather"] = [gather_rate(ctx, n, d, a.launches) for d in (48, 1)]
    for g in result["gather"]:
        print(f"gather d={g['d']:2d}: {g['ms_per_launch'] * 1e3:8.1f} us per launch, "
              f"{g['bytes_per_s'] / 1e12:.3f} TB/s = {g['fraction_of_8TBps']:.3f} of 8 TB/s",
              flush=True)
    for k, v in result["legs"].items():
        print(f"{k:28s} median {v['median_s']:.4f} s ({v['min_s']:.4f} - {v['max_s']:.4f})")
    ctx.close()
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
