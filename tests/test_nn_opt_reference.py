"""The restatement of the line-search optimisers (tests/nn_opt_reference.py)
against hand-worked examples, the branches the parity cases of tests/nn_opt_cases.py reach, the
margin of every decision they take and their float64 noise floor; and the config / model side of
classification.py.  No GPU."""
import collections

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd import classification as clf
from eeg_dataanalysispackage_amd.classification import NN_SEARCH_DTYPE, nn_train_opt
import nn_cases
import nn_opt_cases as cases
import nn_opt_reference as opt
import nn_reference as ref
from test_nn_reference import readme_config

LD = np.longdouble
MARGIN = 1e-8   # every decision of every case is at least this far from its other side
FLOOR = 1e-11   # float64, rows reversed, against long double (the GPU bar is 1e-9)
# a == 0 needs two trials on one exact parabola through (0, s0) with the search's slope; for a
# descent direction Armijo accepts that parabola's minimiser, so only an ascent direction gets
# there, and then only if a network's loss cancels exactly: the synthetic table below reaches it.
SYNTHETIC_ONLY = {"a0:yes"}


def table(values):
    it = iter(values)
    return lambda step: LD(next(it))


def search(values, slope, max_ls=5, s0=0, norm=1, test=1):
    trace = []
    got = opt.line_search(table(values), s0, slope, norm, test, max_ls, trace)
    return got, opt.tags_of(trace)


# ---- line_search by hand --------------------------------------------------------------------------
def test_quadratic_first_backtrack_lands_on_the_minimiser():
    """phi(t) = s0 + m t + c t^2 with s0 = 1, m = -1: phi(1) = c fails Armijo for c > 1 - 1e-4 and
    the backtrack is -m / (2 (phi(1) - s0 - m)) = 1 / (2 c), the parabola's minimiser."""
    seen = []

    def phi(c):
        def f(t):
            seen.append(t)
            return 1 - t + c * t * t
        return f

    for c, want in ((LD(2), LD(1) / 4), (LD(4), LD(1) / 8)):
        del seen[:]
        step, score, trials = opt.line_search(phi(c), 1, -1, 1, 1, 5, [])
        assert seen == [1, want] and step == want and trials == 2
        assert score == 1 - want + c * want * want
    # 1 / (2 c) under a tenth of the step: the 0.1 clamp
    del seen[:]
    opt.line_search(phi(LD(20)), 1, -1, 1, 1, 2, [])
    assert seen == [1, LD(1) / 10]


def test_cubic_on_one_parabola_has_a_zero_and_halves():
    """slope 3, phi(t) = 3 t - 2 t^2 (s0 = 0): phi(1) = 1 is rejected, the backtrack is
    -3 / (2 (1 - 3)) = 3/4; phi(3/4) = 9/8 is rejected; r1 / step^2 = r2 / step2^2 = -2, so a = 0,
    b = -2, tmp = -3 / (2 * -2) = 3/4, cut to half the step: 3/8."""
    seen = []

    def phi(t):
        seen.append(t)
        return 3 * t - 2 * t * t

    trace = []
    opt.line_search(phi, 0, 3, 1, 1, 3, trace)
    assert seen == [1, LD(3) / 4, LD(3) / 8]
    tags = opt.tags_of(trace)
    assert "a0:yes" in tags and "half:clamp" in tags


SYNTHETIC = {
    # name: (values of the trials in order, slope, max_ls, kwargs, (step, score, trials))
    "accept_at_once": ([-1], -1, 5, {}, (1, -1, 1)),
    "min_step_first": ([], -1, 5, dict(test=LD(1) / 10 ** 8), (0, 0, 0)),
    "min_step_later": ([1], -1, 5, dict(test=LD(1) / 10 ** 7 * 3), (0, 0, 1)),
    "rescaled": ([-1], -1, 5, dict(norm=200), (1, -1, 1)),
    "not_finite": ([np.inf, 1, -1], -1, 5, {}, (LD(1) / 25, -1, 3)),
    "nan_never_accepted": ([np.nan] * 3, -1, 3, {}, (0, 0, 3)),
    "cubic": ([1.5, 0.125, -0.25], -1, 5, {}, None),
    "tenth": ([1.5, 1.875, 2.375], -2, 3, {}, (0, 0, 3)),
    "half": ([2.75, 1.375, 0.0], -1, 3, {}, None),
    "disc_negative": ([1.125, 1.25, -0.625, 0.875, 2.375], 2, 5, {}, None),
    "b_not_positive": ([0.875, 1.875, -1.875, 1.75, -1.75], 1, 5, {}, None),
    # lower scores that the steep slope keeps under Armijo's line: the best of them is returned
    "best_step": ([-0.1, -0.2, -0.01], -4096, 3, {},
                  (LD(4096) / (2 * (LD(-0.1) + 4096)), -0.2, 3)),
}


def test_synthetic_tables_reach_every_branch():
    seen = collections.Counter()
    for name, (values, slope, max_ls, kw, want) in SYNTHETIC.items():
        got, tags = search(values, slope, max_ls, **kw)
        seen.update(tags)
        if want is not None:
            assert got[2] == want[2], name
            assert got[0] == LD(want[0]) and got[1] == LD(want[1]), (name, got)
    _, tags = search([1, LD(9) / 8], 3, 2)  # the parabola of the test above, as a table
    seen.update(tags)
    assert set(seen) == set(opt.LINE_TAGS), set(opt.LINE_TAGS) ^ set(seen)


def test_best_step_is_the_step_of_the_lowest_score():
    """slope -4096: Armijo asks for s0 - 0.4096 step.  -0.1 at step 1 falls short of it, the
    backtrack is -m / (2 (phi(1) - m)) = 4096 / (2 * 4095.9); -0.2 there falls short of -0.2048 but
    is the lowest; -0.01 at the third step is higher again."""
    (step, score, trials), tags = search([-0.1, -0.2, -0.01], -4096, 3)
    assert tags.count("lower:yes") == 2 and tags.count("lower:no") == 1 and tags[-1] == "best:yes"
    assert score == LD(-0.2) and trials == 3 and step == LD(4096) / (2 * (LD(-0.1) + 4096))


# ---- directions by hand ---------------------------------------------------------------------------
def test_conjugate_gradient_direction_by_hand():
    g, d = np.array([1, 2, 2], dtype=LD), np.array([1, 0, 0], dtype=LD)
    trace = []
    # dgg = (1, -2, -1) . (2, 0, 1) = 1, gg = 9: gamma = 1/9
    got = opt.cg_direction(g, np.array([2, 0, 1], dtype=LD), d, trace)
    assert np.array_equal(got, np.array([LD(1) / 9 * 1 + 2, 0, 1], dtype=LD))
    # dgg = (-1, -1, -2) . (0, 1, 0) = -1: gamma is cut to 0
    got = opt.cg_direction(g, np.array([0, 1, 0], dtype=LD), d, trace)
    assert np.array_equal(got, np.array([0, 1, 0], dtype=LD))
    assert opt.tags_of(trace) == ["gamma:keep", "gamma:clip"]


def test_lbfgs_direction_by_hand():
    """One pair s = (1, 0, 0), y = (2, 0, 0), g = (4, 2, 0): sy = 2 + EPS, yy = 4 + EPS, rho = 1 /
    sy; a = rho * 4; q = (4 - 2 a, 2, 0) * sy / yy; b = rho * 2 q0; q0 += a - b."""
    eps = LD(1) / 10 ** 5
    sy, yy = 2 + eps, 4 + eps
    a = 4 / sy
    q0 = (4 - 2 * a) * (sy / yy)
    want = np.array([q0 + (a - 2 * q0 / sy), 2 * (sy / yy), 0], dtype=LD)
    history, trace = [], []
    got = opt.lbfgs_direction(history, np.array([1, 0, 0], dtype=LD), np.array([2, 0, 0], dtype=LD),
                              np.array([4, 2, 0], dtype=LD), trace)
    assert np.allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64),
                       rtol=1e-15, atol=0)
    assert abs(got[0] - want[0]) <= 4 * np.finfo(LD).eps * abs(want[0])
    # the history keeps the newest HISTORY pairs, newest first
    for k in range(opt.HISTORY + 1):
        opt.lbfgs_direction(history, np.array([k + 2, 0, 0], dtype=LD),
                            np.array([1, 0, 0], dtype=LD), np.array([1, 1, 1], dtype=LD), trace)
    assert len(history) == opt.HISTORY and history[0][0][0] == opt.HISTORY + 2
    assert opt.tags_of(trace)[-2:] == ["history:full", "history:full"]


def test_search_constants_by_hand():
    p = np.array([0.5, -4, 1], dtype=LD)
    g = np.array([3, 8, -1], dtype=LD)
    d = np.array([3, 4, 0], dtype=LD)
    norm, slope, test = opt.search_constants(p, g, d)
    assert norm == 5 and slope == -41 and test == 3   # max(3 / 1, 8 / 4, 1 / 1)
    g[1] = np.nan
    assert np.isnan(opt.search_constants(p, g, d)[2])


# ---- the cases ------------------------------------------------------------------------------------
def test_the_cases_the_issue_names_are_there():
    c = cases.CASES
    for a in ("line", "cg", "lbfgs"):
        for u in ("sgd", "nesterovs", "adam"):
            k = c[f"{a}_{u}"]
            assert (k["n"], k["d"], k["widths"]) == (203, 48, (8, 2)) and k["iterations"] >= 6
    rows, _ = nn_cases.plan_tile(5, (3, 2))
    assert {k["n"] for k in c.values() if (k["d"], k["widths"]) == (5, (3, 2))} == \
        {1, rows - 1, rows + 1}
    trip = c["cg_second_trip"]
    assert trip["n"] == nn_cases.TRIP_ROWS + 1 and trip["last_row_only"]
    assert nn_cases.grid(trip["n"], 1, (1, 2)) == nn_cases.constants()["kNnGridCap"]
    wide = c["lbfgs_wide_d"]
    assert wide["d"] == nn_cases.LAST_STAGED_D + 1 and wide["widths"] == (64, 2)
    assert not nn_cases.plan_tile(wide["d"], wide["widths"])[1]
    counts = {ref.param_count(k["d"], k["widths"]) for k in c.values()}
    threads = nn_cases.constants()["kNnDirThreads"]
    assert {4, 255, 256, 257, threads - 1, threads, threads + 1, 74050} <= counts
    assert {k["max_ls"] for k in c.values()} >= {1, 5}
    assert any(k["nan_row"] is not None for k in c.values())
    assert c["cg_lr1e-9"]["learning_rate"] == 1e-9


def test_the_cases_reach_every_branch_a_network_can_reach():
    seen = collections.Counter()
    for name in cases.CASES:
        seen.update(opt.tags_of(cases.reference(name)["trace"]))
    assert set(seen) == set(opt.TAGS) - SYNTHETIC_ONLY, set(seen) ^ set(opt.TAGS)


def test_named_cases_do_what_they_are_named_for():
    tags = lambda name: set(opt.tags_of(cases.reference(name)["trace"]))
    assert "history:full" in tags("lbfgs_sgd") and "history:full" in tags("lbfgs_adam")
    assert {"finite:no", "rescale:yes", "best:yes"} <= tags("line_xent_saturates")
    r = cases.reference("cg_lr1e-9")
    assert r["trials"].tolist() == [0] and r["steps"].tolist() == [0]
    assert "eps:stop" in tags("cg_lr1e-9")
    for a in ("line", "cg", "lbfgs"):
        r = cases.reference(f"{a}_nan_row")
        assert r["trials"].tolist() == [5, 5] and not r["steps"].any()
        assert np.isnan(np.asarray(r["scores"], dtype=np.float64)).all()
    r = cases.reference("lbfgs_zero_direction")
    assert r["iterations_run"] == 1 and "zero:stop" in tags("lbfgs_zero_direction")
    assert {"disc:neg", "b:nonpos", "half:clamp"} <= tags("cg_relu_lr3") | tags("cg_tanh_lr10")
    assert "gamma:clip" in tags("cg_sgd") and "tenth:clamp" in tags("lbfgs_n_65")
    assert cases.reference("cg_lr30_one_trial")["trials"].max() == 1
    for a in ("line", "cg", "lbfgs"):  # every algorithm lowers the loss
        s = cases.reference(f"{a}_sgd")["scores"]
        assert s[-1] < s[0]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_decision_has_a_margin(name):
    m, tag = opt.smallest_margin(cases.reference(name)["trace"])
    print(f"{name}: closest decision {m:.3e} at {tag}")
    assert m >= MARGIN


def rel(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    return float(np.linalg.norm(got[finite] - want[finite]) /
                 max(np.linalg.norm(want[finite]), LD(1e-300)))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_noise_floor_and_decisions_of_the_float64_run(name):
    """A float64 run with the rows summed in reversed order takes the decisions of the long-double
    run and stays within 1e-11 (relative) of it: a 100x margin under the GPU bar of 1e-9."""
    want, got = cases.reference(name), cases.reference64(name)
    assert opt.tags_of(got["trace"]) == opt.tags_of(want["trace"])
    assert got["iterations_run"] == want["iterations_run"]
    assert got["trials"].tolist() == want["trials"].tolist()
    for k in ("params", "scores", "steps", "search_scores"):
        e = rel(got[k], want[k])
        print(f"{name} {k}: {e:.3e}")
        assert e <= FLOOR


# ---- classification.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", opt.ALGORITHMS)
def test_config_with_line_search_accepts_the_three(algo):
    c = readme_config()
    c["config_optimization_algo"] = algo
    m = clf.nn_config_from(c, 48, line_search=True)
    assert m.optimization_algo == algo and m.max_line_search_iterations == 5
    assert m.optimizer().algorithm == _lib.NN_OPTIMIZERS[algo]
    with pytest.raises(fx.EegfxError) as e:  # the two-argument call keeps refusing them
        clf.nn_config_from(c, 48)
    assert e.value.code == _lib.EEGFX_ENOTSUP and algo in str(e.value)


def test_readme_defaults_yield_conjugate_gradient():
    """The reference's README: config_optimization_algo -> default = conjugate_gradient."""
    c = readme_config()
    c["config_optimization_algo"] = "conjugate_gradient"
    m = clf.nn_config_from(c, 48, line_search=True)
    assert m.optimization_algo == "conjugate_gradient"
    assert m == clf.NnModel(d=48, widths=(16, 2), activations=("relu", "sigmoid"), loss="xent",
                            updater="nesterovs", learning_rate=0.1, momentum=0.5,
                            num_iterations=1000, seed=12345, weight_init="xavier",
                            optimization_algo="conjugate_gradient")


def test_unknown_optimiser_strings_still_map_to_sgd():
    c = readme_config()
    for algo in ("sgd", "hessian_free", ""):
        c["config_optimization_algo"] = algo
        for flag in (False, True):
            assert clf.nn_config_from(c, 48, flag).optimization_algo == "stochastic_gradient_descent"
    assert clf.NnModel(d=1, widths=(2,), activations=("sigmoid",)).optimizer().algorithm == \
        _lib.NN_OPTIMIZERS["stochastic_gradient_descent"]


def test_binding_matches_the_header():
    assert _lib.NN_OPTIMIZERS == {"stochastic_gradient_descent": 0, "line_gradient_descent": 1,
                                  "conjugate_gradient": 2, "lbfgs": 3}
    import ctypes
    assert ctypes.sizeof(_lib.NnSearch) == 24 == NN_SEARCH_DTYPE.itemsize
    assert ctypes.sizeof(_lib.NnOptimizer) == 8
    assert "eegfx_nn_train_opt" in _lib.SIGNATURES and hasattr(fx, "nn_train_opt")
