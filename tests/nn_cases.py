"""The parity cases of train_clf=nn, shared by the CPU tests (noise floor, dispatch) and the GPU
tests (parity with tests/nn_reference.py), with the kernels' tiling restated from the named
constants at the top of csrc/nn.hip."""
import functools
import os
import re

import numpy as np

import nn_reference as ref
from conftest import REPO

NN_HIP = os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc", "nn.hip")


@functools.lru_cache(maxsize=None)
def constants():
    """Every `constexpr int kNn... = <number>;` of nn.hip."""
    text = open(NN_HIP).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (kNn\w+) = (\d+);", text)}


def plan_tile(d, widths):
    """nn_plan_tile restated: (rows of a tile, whether layer 1's weights are staged in LDS)."""
    c = constants()
    odd = lambda v: v | 1
    shapes = ref.layer_shapes(d, widths)
    per_row = odd(d) + 2 + sum(2 * odd(o) for _, o in shapes)
    fixed = c["kNnMaxTileRows"] + sum(o for _, o in shapes)
    fixed += sum(i * odd(o) for i, o in shapes[1:])
    budget = c["kNnLdsBytes"] // 8
    w1 = shapes[0][0] * odd(shapes[0][1])
    staged = budget - fixed - w1 >= c["kNnMinStagedRows"] * per_row
    if staged:
        fixed += w1
    return min(c["kNnMaxTileRows"], (budget - fixed) // per_row), staged


def grid(n, d, widths):
    """nn_grid restated: the workgroups of nn_grad_kernel."""
    c = constants()
    rows, _ = plan_tile(d, widths)
    cap = min(c["kNnGridCap"], max(1, c["kNnPartialDoubles"] // (ref.param_count(d, widths) + 1)))
    return max(1, min((n + rows - 1) // rows, cap))


def case(n, d, widths, hidden="tanh", out="softmax", loss="negativeloglikelihood",
         updater="nesterovs", iterations=3, last_row_only=False, activations=None):
    acts = tuple(activations) if activations else (hidden,) * (len(widths) - 1) + (out,)
    return dict(n=n, d=d, widths=tuple(widths), activations=acts, loss=loss, updater=updater,
                iterations=iterations, learning_rate=0.1, momentum=0.5,
                last_row_only=last_row_only)


def _cases():
    c = {}
    for u in ("sgd", "nesterovs", "adam", "adagrad", "rmsprop"):
        c[f"updater_{u}"] = case(203, 48, (8, 2), updater=u, iterations=5)
    for a in ("sigmoid", "tanh", "relu", "identity", "softplus", "elu", "softmax"):
        c[f"hidden_{a}"] = case(67, 5, (4, 2), hidden=a, out="sigmoid", loss="mse")
    for loss, out in (("xent", "sigmoid"), ("negativeloglikelihood", "softmax"),
                      ("mse", "sigmoid"), ("squared_loss", "identity"), ("xent", "softmax"),
                      ("mse", "softmax"), ("negativeloglikelihood", "sigmoid"),
                      ("squared_loss", "tanh")):
        c[f"loss_{loss}_{out}"] = case(67, 5, (4, 2), out=out, loss=loss)
    for widths in ((2,), (5, 2), (5, 4, 2), (5, 4, 3, 2)):
        c[f"layers_{len(widths)}"] = case(67, 5, widths)
    for w in (1, 2, 16, 17, 63, 64):
        c[f"width_{w}"] = case(67, 5, (w, 2))
    c["widest_4_layers"] = case(40, 48, (64, 64, 64, 2), iterations=2)
    for d in (1, 16, 17, 48, 64, 65, 512, 1024):
        c[f"d_{d}"] = case(37, d, (4, 2), iterations=2)
    # layer 1 at width 64: staged in LDS up to LAST_STAGED_D features, read through L2 past it
    for d in (1, LAST_STAGED_D, LAST_STAGED_D + 1, 512, 1024):
        c[f"wide_d_{d}"] = case(37, d, (64, 2), iterations=2)
    rows, _ = plan_tile(5, (3, 2))
    for n in (1, rows - 1, rows, rows + 1, 2 * rows + 1):
        c[f"n_{n}"] = case(n, 5, (3, 2))
    # one full trip of the capped grid and one row: only the last row has a feature that is not 0
    rows, _ = plan_tile(1, (1, 2))
    trip = constants()["kNnGridCap"] * rows
    for n in (trip - 1, trip, trip + 1):
        c[f"trip_{n}"] = case(n, 1, (1, 2), iterations=1, last_row_only=True)
    return c


def _last_staged_d(width):
    d = 1
    while plan_tile(d + 1, (width, 2))[1]:
        d += 1
    return d


LAST_STAGED_D = _last_staged_d(64)
CASES = _cases()
TRIP_ROWS = constants()["kNnGridCap"] * plan_tile(1, (1, 2))[0]


def spec_of(c):
    return {k: c[k] for k in ("d", "widths", "activations", "loss", "updater", "learning_rate",
                              "momentum")}


@functools.lru_cache(maxsize=None)
def data(name):
    """(X, y, params0) of a case: standard normal rows, labels from a planted direction, Xavier
    weights with zero biases.  Read-only."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    X = rng.standard_normal((c["n"], c["d"]))
    y = (X @ rng.standard_normal(c["d"]) + 0.3 * rng.standard_normal(c["n"]) > 0).astype(np.float64)
    if c["last_row_only"]:
        X[:-1] = 0.0
        X[-1] = 1.5
        y = (np.arange(c["n"]) % 3 == 0).astype(np.float64)
    parts = []
    for n_in, n_out in ref.layer_shapes(c["d"], c["widths"]):
        parts += [rng.standard_normal(n_in * n_out) * np.sqrt(2.0 / (n_in + n_out)),
                  np.zeros(n_out)]
    p0 = np.concatenate(parts)
    for a in (X, y, p0):
        a.setflags(write=False)
    return X, y, p0


@functools.lru_cache(maxsize=None)
def reference(name):
    """(params, scores, predictions under the trained params) of a case in long double, once."""
    c = CASES[name]
    X, y, p0 = data(name)
    p, scores = ref.train(p0, X, y, spec_of(c), c["iterations"])
    return p, scores, ref.predict(p, X, spec_of(c))
