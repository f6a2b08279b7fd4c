"""Prints the bits the one-context SGD trainers return, to compare two builds of libeegfx.so
(outputs in profiles/one_sgd_driver/).

  python tools/sgd_bits.py [--lib PATH] [--rows 1,63,300,2100,32769] [--sha256]

eegfx_logreg_sgd_train_partitioned (4 partitions; mini-batch fractions 1.0, 0.5 and 0.03) and
eegfx_svm_sgd_train (full batch) on the same rows for every n of --rows and every d of WIDTHS, each
with convergence tolerance 0.001 (up to 1000 iterations, so that a run can converge and leave the
rest of its launches empty) and with tolerance 0 (all of 100 iterations run), the rows in host
memory and on the device.  The first line names the library; then one JSON line per case with
iterations_run and the weights as the hex of their bytes (--sha256: the digest of those bytes, for
an output small enough to keep: the hex of all 560 cases is 2 MB).  The case lines do not depend on --lib's
path, so the outputs of two builds on one GPU are compared with diff."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "eeg_dataanalysispackage_amd", "libeegfx.so")
ROWS = "1,63,300,2100,32769"              # the last: one row past lr_grid's cap of 512 workgroups
WIDTHS = (1, 16, 48, 128, 129, 257, 1024)  # first and last width of each kernel's buckets
STOPS = ((0.001, 1000), (0.0, 100))         # (convergence tolerance, iterations)
PARTS, MEM_HOST, MEM_DEVICE = 4, 0, 1
KINDS = (("logistic", 1.0), ("logistic", 0.5), ("logistic", 0.03), ("hinge", 1.0))


def check(lib, rc):
    if rc != 0:
        lib.eegfx_last_error.restype = ctypes.c_char_p
        sys.exit(f"status {rc}: {lib.eegfx_last_error().decode()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--rows", default=ROWS)
    ap.add_argument("--sha256", action="store_true")
    a = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    print(json.dumps({"lib": os.path.relpath(os.path.abspath(a.lib)), "rows": a.rows,
                      "partitions": PARTS}))
    ctx = ctypes.c_void_p()
    check(lib, lib.eegfx_ctx_create(0, ctypes.byref(ctx)))
    dbl, i32, i64, vp = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    for n in (int(v) for v in a.rows.split(",")):
        for d in WIDTHS:
            rng = np.random.default_rng(1000 * d + n)
            X = rng.standard_normal((n, d))
            X /= np.linalg.norm(X, axis=1, keepdims=True)
            y = (X @ rng.standard_normal(d) > 0).astype(np.float64)
            start = 0.01 * rng.standard_normal(d)
            Xd, yd = torch.from_numpy(X).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
            torch.cuda.synchronize()
            for mem, px, py in ((MEM_HOST, X.ctypes.data, y.ctypes.data),
                                (MEM_DEVICE, Xd.data_ptr(), yd.data_ptr())):
                for kind, fraction in KINDS:
                    for tol, iters in STOPS:
                        w = start.copy()
                        it = i32(-1)
                        head = (ctx, vp(px), vp(py), i64(n), i32(d), i32(iters), dbl(1.0),
                                dbl(0.01), dbl(fraction), dbl(tol))
                        tail = (vp(w.ctypes.data), ctypes.byref(it), mem)
                        if kind == "hinge":
                            check(lib, lib.eegfx_svm_sgd_train(*head, *tail))
                        else:
                            check(lib, lib.eegfx_logreg_sgd_train_partitioned(*head, i32(PARTS),
                                                                              *tail))
                        bits = ({"weights_sha256": hashlib.sha256(w.tobytes()).hexdigest()}
                                if a.sha256 else {"weights": w.tobytes().hex()})
                        print(json.dumps({"kind": kind, "n": n, "d": d, "fraction": fraction,
                                          "tol": tol, "iterations": iters,
                                          "mem": "device" if mem else "host",
                                          "iterations_run": it.value, **bits}))
            del Xd, yd
    check(lib, lib.eegfx_ctx_destroy(ctx))


if __name__ == "__main__":
    main()
