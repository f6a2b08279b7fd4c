"""Times the SGD trainer over shards against the one-context entry.

  python tools/measure_sharded_sgd.py [--lib PATH] [--rows N] [--shards 1,2,4] [--repeats R]

Full batch, 100 iterations, d = 48, convergence tolerance 0 (every iteration runs), rows resident
on the device.  Wall clock around the call, which drains every context before it returns; 3
warm-up calls, then the median, minimum and maximum of R calls.  --lib names another build of
libeegfx.so (a parent commit's: only the one-context entry is timed there).  Context i is created
on device i % device count; the first line of the output says how many devices there are, so
whether the shards of a k > 1 run shared one GPU.  Prints one JSON line per timing."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "eeg_dataanalysispackage_amd", "libeegfx.so")
D, ITERS, MEM_DEVICE = 48, 100, 1


class GlmShard(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("X", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("pos", ctypes.c_void_p), ("n", ctypes.c_int64)]


def check(lib, rc):
    if rc != 0:
        lib.eegfx_last_error.restype = ctypes.c_char_p
        sys.exit(f"status {rc}: {lib.eegfx_last_error().decode()}")


def timed(call, repeats):
    for _ in range(3):
        call()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--shards", default="1,2,4")
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    sharded = hasattr(lib, "eegfx_glm_sgd_train_sharded")
    ks = [int(k) for k in a.shards.split(",")] if sharded else []
    n_dev = torch.cuda.device_count()
    print(json.dumps({"lib": os.path.relpath(os.path.abspath(a.lib)), "devices": n_dev,
                      "rows": a.rows, "d": D, "iterations": ITERS}))
    ctxs = []
    for i in range(max(ks + [1])):
        h = ctypes.c_void_p()
        check(lib, lib.eegfx_ctx_create(i % n_dev, ctypes.byref(h)))
        ctxs.append((h, i % n_dev))
    g = torch.Generator(device="cuda:0").manual_seed(7)
    X = torch.randn((a.rows, D), dtype=torch.float64, device="cuda:0", generator=g)
    X /= X.norm(dim=1, keepdim=True)
    w0 = torch.randn(D, dtype=torch.float64, device="cuda:0", generator=g)
    y = (X @ w0 > 0).to(torch.float64)
    torch.cuda.synchronize()
    w = (ctypes.c_double * D)()
    it = ctypes.c_int32()
    dbl, i32, i64 = ctypes.c_double, ctypes.c_int32, ctypes.c_int64

    def one_context():
        for j in range(D):
            w[j] = 0.0
        check(lib, lib.eegfx_logreg_sgd_train(ctxs[0][0], ctypes.c_void_p(X.data_ptr()),
                                              ctypes.c_void_p(y.data_ptr()), i64(a.rows), i32(D),
                                              i32(ITERS), dbl(1.0), dbl(0.01), dbl(1.0), dbl(0.0),
                                              w, ctypes.byref(it), MEM_DEVICE))
        assert it.value == ITERS

    print(json.dumps({"entry": "eegfx_logreg_sgd_train", **timed(one_context, a.repeats)}))
    want = list(w)
    for k in ks:
        parts, off = [], 0
        for s in range(k):
            m = a.rows // k + (1 if s < a.rows % k else 0)
            dev = f"cuda:{ctxs[s][1]}"
            parts.append((X[off:off + m].to(dev).contiguous(), y[off:off + m].to(dev).contiguous()))
            off += m
        torch.cuda.synchronize()
        arr = (GlmShard * k)(*[GlmShard(ctxs[s][0], xs.data_ptr(), ys.data_ptr(), None,
                                        xs.shape[0]) for s, (xs, ys) in enumerate(parts)])

        def over_shards():
            for j in range(D):
                w[j] = 0.0
            check(lib, lib.eegfx_glm_sgd_train_sharded(0, arr, i32(k), i32(D), i32(ITERS),
                                                       dbl(1.0), dbl(0.01), dbl(1.0), dbl(0.0),
                                                       i32(1), w, ctypes.byref(it)))
            assert it.value == ITERS

        r = timed(over_shards, a.repeats)
        err = max(abs(p - q) for p, q in zip(w, want)) / max(abs(q) for q in want)
        print(json.dumps({"entry": "eegfx_glm_sgd_train_sharded", "shards": k,
                          "same_bits_as_one_context": list(w) == want,
                          "max_rel_to_one_context": err, **r}))
        del parts, arr


if __name__ == "__main__":
    main()
