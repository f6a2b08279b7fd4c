#!/usr/bin/env python3
"""Times OffLineDataProvider.loadData over a directory of recordings: eegfx_odp_create's
one-context provider (the baseline) against eegfx_odp_create_multi with 1, 2, 4 and 8 contexts
spread over the visible devices (context i on device i % device_count).

Writes --files synthetic int16 recordings of --frames frames x 3 channels with a marker every
--spacing frames into a temporary directory, loads them once to warm the page cache, then reports
the median, minimum and maximum of --repeat loads per leg.  Recorded, with no threshold: on a box
with one GPU the multi legs show only the overlap of file reads, uploads and kernels.

    python tools/odp_multi_bench.py [--lib path/to/libeegfx.so] [--files 64] [--frames 1000000]
                                    [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import eeg_dataanalysispackage_amd as fx  # noqa: E402
from eeg_dataanalysispackage_amd import _lib  # noqa: E402


def write_directory(root, files, frames, spacing):
    rng = np.random.default_rng(7)
    block = np.clip(np.cumsum(rng.integers(-40, 41, size=(frames, 3)), axis=0) - 25000,
                    -32768, 32767).astype("<i2")
    names = []
    for f in range(files):
        name = f"rec{f:03d}"
        np.roll(block, 997 * f, axis=0).tofile(os.path.join(root, name + ".eeg"))
        with open(os.path.join(root, name + ".vhdr"), "w", encoding="utf-8") as h:
            h.write("Brain Vision Data Exchange Header File Version 1.0\n\n[Common Infos]\n"
                    f"Codepage=UTF-8\nDataFile={name}.eeg\nMarkerFile={name}.vmrk\n"
                    "DataFormat=BINARY\nDataOrientation=MULTIPLEXED\nNumberOfChannels=3\n"
                    "SamplingInterval=1000\n\n[Binary Infos]\nBinaryFormat=INT_16\n\n"
                    "[Channel Infos]\nCh1=Fz,,0.1,µV\nCh2=Cz,,0.1,µV\nCh3=Pz,,0.1,µV\n")
        with open(os.path.join(root, name + ".vmrk"), "w", encoding="utf-8") as m:
            m.write("Brain Vision Data Exchange Marker File, Version 1.0\n\n[Common Infos]\n"
                    f"Codepage=UTF-8\nDataFile={name}.eeg\n\n[Marker Infos]\n"
                    "Mk1=New Segment,,1,1,0,20150128095308551177\n")
            # target / non-target alternate: the balanced selection keeps every marker
            for i, p in enumerate(range(spacing, frames, spacing)):
                m.write(f"Mk{i + 2}=Stimulus,S  {1 + i % 2},{p},1,0\n")
        names.append(name)
    info = os.path.join(root, "info.txt")
    with open(info, "w") as f:
        f.write("".join(f"{n}.eeg 1\n" for n in names))
    return info


def time_leg(make, repeat):
    times, n = [], 0
    for _ in range(repeat + 1):          # the first load warms the page cache and the buffers
        odp = make()
        t0 = time.perf_counter()
        odp.loadData()
        times.append(time.perf_counter() - t0)
        assert odp.last_error == "", odp.last_error
        n = odp.num_epochs()
        odp.close()
    times = times[1:]
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times),
            "epochs": n}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=None, help="libeegfx.so to load (default: the package's)")
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--spacing", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--contexts", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    n_dev = fx.device_count()
    result = {"lib": a.lib or "package", "devices": n_dev, "files": a.files, "frames": a.frames, "spacing": a.spacing,
              "repeat": a.repeat, "legs": {}}
    with tempfile.TemporaryDirectory() as root:
        info = write_directory(root, a.files, a.frames, a.spacing)
        ctxs = [fx.Context(i % n_dev) for i in range(max(a.contexts + [1]))]
        legs = [("odp_create", lambda: fx.OffLineDataProvider([info], context=ctxs[0]))]
        for k in a.contexts:
            legs.append((f"odp_create_multi_{k}",
                         lambda k=k: fx.OffLineDataProvider([info], contexts=ctxs[:k])))
        for name, make in legs:
            result["legs"][name] = time_leg(make, a.repeat)
            print(f"{name:24s} median {result['legs'][name]['median_s'] * 1e3:9.1f} ms   "
                  f"min {result['legs'][name]['min_s'] * 1e3:9.1f}   "
                  f"max {result['legs'][name]['max_s'] * 1e3:9.1f}   "
                  f"epochs {result['legs'][name]['epochs']}", flush=True)
        for c in ctxs:
            c.close()
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
