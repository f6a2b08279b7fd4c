"""The parity cases of the line-search optimisers of train_clf=nn, shared
by the CPU tests (branch coverage, margins, noise floor) and the GPU tests (parity with
tests/nn_opt_reference.py), in the style of tests/nn_cases.py, whose tiling they reuse."""
import functools
import zlib

import numpy as np

import nn_cases
import nn_opt_reference as opt
import nn_reference as ref

SHORT = {"line_gradient_descent": "line", "conjugate_gradient": "cg", "lbfgs": "lbfgs"}


def case(algorithm, n, d, widths, iterations, max_ls=5, learning_rate=0.1, momentum=0.5,
         nan_row=None, zero_start=False, seed=None, **kw):
    c = nn_cases.case(n, d, widths, iterations=iterations, **kw)
    c.update(algorithm=algorithm, max_ls=max_ls, learning_rate=learning_rate, momentum=momentum,
             nan_row=nan_row, zero_start=zero_start, seed=seed)
    return c


def _cases():
    c = {}
    algos = opt.ALGORITHMS
    # every algorithm under three updaters; 6 iterations push 6 pairs: the LBFGS history overflows
    for a in algos:
        for u in ("sgd", "nesterovs", "adam"):
            c[f"{SHORT[a]}_{u}"] = case(a, 203, 48, (8, 2), 6, updater=u)
    # a learning rate that makes the first step too long: backtracking (quadratic, cubic, the 0.1
    # clamp), the direction rescaled to stepMax, a slope that the rescale leaves too steep for
    # Armijo (max-trials exits, with and without a better score)
    for a in algos:
        c[f"{SHORT[a]}_lr30_nll"] = case(a, 203, 48, (8, 2), 8, updater="sgd", learning_rate=30.0)
    for a in ("line_gradient_descent", "lbfgs"):
        c[f"{SHORT[a]}_lr30"] = case(a, 203, 48, (8, 2), 8, updater="sgd", learning_rate=30.0,
                                     out="sigmoid", loss="xent")
    # a cubic with a negative discriminant, with b <= 0, and a minimiser past 0.5 step
    small = dict(n=67, d=5, widths=(4, 2), iterations=6, updater="sgd")
    c["cg_relu_lr3"] = case("conjugate_gradient", learning_rate=3.0, hidden="relu", seed=0, **small)
    c["cg_tanh_lr10"] = case("conjugate_gradient", learning_rate=10.0, seed=4, **small)
    c["lbfgs_relu_mse_lr3"] = case("lbfgs", learning_rate=3.0, hidden="relu", out="sigmoid",
                                   loss="mse", seed=0, **{**small, "updater": "nesterovs"})
    c["cg_lr30_one_trial"] = case("conjugate_gradient", 203, 48, (8, 2), 4, max_ls=1,
                                  updater="sgd", learning_rate=30.0, out="sigmoid", loss="xent")
    c["lbfgs_lr3_two_trials"] = case("lbfgs", 203, 48, (8, 2), 6, max_ls=2, updater="sgd",
                                     learning_rate=3.0)
    # xent: a step that drives a sigmoid output to 1 where the label is 0 -- a non-finite score
    c["line_xent_saturates"] = case("line_gradient_descent", 67, 5, (4, 2), 3, updater="sgd",
                                    learning_rate=1e4, out="sigmoid", loss="xent")
    c["lbfgs_xent_saturates"] = case("lbfgs", 67, 5, (4, 2), 3, updater="sgd",
                                     learning_rate=1e4, out="sigmoid", loss="xent")
    # 1 < stepMin at the first check of every search
    c["cg_lr1e-9"] = case("conjugate_gradient", 67, 5, (4, 2), 2, updater="sgd",
                          learning_rate=1e-9)
    # one NaN feature: every score is a NaN (and the test of stepMin: no step is too small), every
    # search backs off through its trials and returns 0
    for a in algos:
        c[f"{SHORT[a]}_nan_row"] = case(a, 67, 5, (4, 2), 2, updater="adam", nan_row=40)
    # zero parameters, balanced labels, mse over sigmoid: the gradient is exactly zero
    c["lbfgs_zero_direction"] = case("lbfgs", 64, 5, (4, 2), 3, updater="sgd", out="sigmoid",
                                     loss="mse", zero_start=True)
    rows, _ = nn_cases.plan_tile(5, (3, 2))
    for n, a in zip((1, rows - 1, rows + 1), algos):
        c[f"{SHORT[a]}_n_{n}"] = case(a, n, 5, (3, 2), 3)
    # the score kernel's second grid trip: the one row with a feature lies there
    c["cg_second_trip"] = case("conjugate_gradient", nn_cases.TRIP_ROWS + 1, 1, (1, 2), 1,
                               last_row_only=True)
    # the candidate's layer 1 is read through L2
    c["lbfgs_wide_d"] = case("lbfgs", 37, nn_cases.LAST_STAGED_D + 1, (64, 2), 2)
    # the direction kernel's reductions: P = 4, and just below, at and above 256 and 1024
    for (d, widths), a in zip(((1, (2,)), (20, (11, 2)), (127, (2,)), (14, (15, 2)),
                               (1018, (1, 2)), (511, (2,)), (28, (33, 2))), algos * 3):
        P = ref.param_count(d, widths)
        c[f"{SHORT[a]}_P_{P}"] = case(a, 23, d, widths, 3)
    c["lbfgs_P_74050"] = case("lbfgs", 19, 1024, (64, 64, 64, 2), 2)
    return c


CASES = _cases()


def spec_of(c):
    return nn_cases.spec_of(c)


@functools.lru_cache(maxsize=None)
def data(name):
    """(X, y, params0) of a case, as nn_cases.data draws them; nan_row: one NaN feature in that
    row; zero_start: zero parameters and labels 0, 1, 0, 1, ...  Read-only."""
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) if c["seed"] is None else c["seed"])
    X = rng.standard_normal((c["n"], c["d"]))
    y = (X @ rng.standard_normal(c["d"]) + 0.3 * rng.standard_normal(c["n"]) > 0).astype(np.float64)
    if c["last_row_only"]:
        X[:-1] = 0.0
        X[-1] = 1.5
        y = (np.arange(c["n"]) % 3 == 0).astype(np.float64)
    if c["nan_row"] is not None:
        X[c["nan_row"], c["d"] // 2] = np.nan
    parts = []
    for n_in, n_out in ref.layer_shapes(c["d"], c["widths"]):
        parts += [rng.standard_normal(n_in * n_out) * np.sqrt(2.0 / (n_in + n_out)),
                  np.zeros(n_out)]
    p0 = np.concatenate(parts)
    if c["zero_start"]:
        p0[:] = 0.0
        y = (np.arange(c["n"]) % 2).astype(np.float64)
    for a in (X, y, p0):
        a.setflags(write=False)
    return X, y, p0


@functools.lru_cache(maxsize=None)
def reference(name):
    """nn_opt_reference.train_opt of a case in long double, once."""
    return run(name)


@functools.lru_cache(maxsize=None)
def reference64(name):
    """... and in float64 with the rows summed from the last to the first."""
    return run(name, dtype=np.float64, reverse=True)


def run(name, **kw):
    c = CASES[name]
    X, y, p0 = data(name)
    return opt.train_opt(p0, X, y, spec_of(c), c["algorithm"], c["iterations"], c["max_ls"], **kw)
