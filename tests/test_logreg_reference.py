"""oracle/mllib_logreg.py (float64, the judge of the GPU classifier tests) pinned against the
independent long-double restatement of tests/logreg_reference.py, on every training and prediction
shape test_gpu_logreg_shapes.py uses -- both gradients, full batch and mini-batch:

  the same iteration count, and ||w_oracle - w_ld|| <= 1e-12 ||w_ld|| (measured 3e-16 .. 8e-15:
  the bound leaves two orders for BLAS and summation-order differences between machines);

and the conditions under which a float64 loop can be compared with another one at all, stated for
the long-double run alone:

  conv_margin >= 1e-4   no convergence test within 1e-4 (relative) of flipping;
  hinge_gap   >= 1e-6   no row within 1e-6 of changing side of the hinge in any iteration.

A case that misses a condition gets another seed or step (logreg_reference._SEED / _STEP), never
another bound.  Non-finite feature rows: HingeGradient skips a row whose margin is NaN, so the
hinge weights stay finite through a NaN entry; LogisticGradient has no such branch.
"""
import numpy as np
import pytest

import logreg_reference as lr
from oracle import mllib_logreg as ref

ORACLE_REL = 1e-12
CONV_MARGIN = 1e-4
HINGE_GAP = 1e-6
# scores and margins: a tenth of the 1e-12 the GPU tests allow the device against this oracle, so
# the oracle can judge at that bar (a float64 dot product of d <= 1024 terms of ||x|| = 1,
# ||w|| <= 70 rounds within about sqrt(d) 2^-53 ||w|| = 2.5e-13 at the very worst shape)
PREDICT_ABS = 1e-13


def norm(v):
    v = np.asarray(v, dtype=lr.LD)
    return np.sqrt((v * v).sum())


def ld_run(c, X, y):
    sample = None
    if c.fraction < 1.0:
        def sample(i):
            return ref.sample_rows(c.n, c.fraction, c.parts, 42 + i)
    return lr.sgd_train(X, y, c.iters, c.step, c.reg, initial=lr.case_start(c),
                        gradient=c.gradient, rows_of_iteration=sample)


def oracle_run(c, X, y):
    return ref.sgd_train(X, y, c.iters, c.step, c.reg, initial=lr.case_start(c),
                         gradient=c.gradient, mini_batch_fraction=c.fraction,
                         num_partitions=c.parts)


def test_rows_is_the_generator_of_test_gpu_logreg():
    """logreg_reference.rows restates test_gpu_logreg.rows (that module needs torch to import)."""
    import ast
    import inspect
    import os
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_logreg.py")).read()
    theirs = next(f for f in ast.parse(src).body
                  if isinstance(f, ast.FunctionDef) and f.name == "rows")
    ours = ast.parse(inspect.getsource(lr.rows)).body[0]
    assert [ast.dump(s) for s in theirs.body[1:]] == [ast.dump(s) for s in ours.body[1:]]


@pytest.mark.parametrize("c", lr.ALL_CASES, ids=lr.case_id)
def test_oracle_matches_long_double(c):
    X, y = lr.case_rows(c)
    ld = ld_run(c, X, y)
    w, it = oracle_run(c, X, y)
    err = float(norm(w.astype(lr.LD) - ld.weights) / norm(ld.weights))
    print(f"{lr.case_id(c)}: iterations {it} / {ld.iterations}  rel {err:.2e}  "
          f"conv_margin {ld.conv_margin:.3e}  hinge_gap {ld.hinge_gap:.3e}")
    assert ld.conv_margin >= CONV_MARGIN
    if c.gradient == "hinge":
        assert ld.hinge_gap >= HINGE_GAP
    assert it == ld.iterations
    assert err <= ORACLE_REL


def test_the_empty_sample_case_has_empty_samples():
    n, d = lr.EMPTY_SAMPLE_ND
    assert d != 48
    empty = [i for i in range(1, 101) if not ref.sample_rows(n, 0.03, 4, 42 + i)]
    assert empty and len(empty) < 100


def test_zero_iterations_and_initial_weights():
    X, y = lr.rows(50, 7, 3)
    start = lr.initial_weights(7)
    keep = start.copy()
    for g in lr.GRADIENTS:
        w, it = ref.sgd_train(X, y, 0, initial=start, gradient=g)
        r = lr.sgd_train(X, y, 0, initial=start, gradient=g)
        assert it == r.iterations == 0
        assert np.array_equal(w, keep) and np.array_equal(r.weights.astype(np.float64), keep)
        ref.sgd_train(X, y, 5, initial=start, gradient=g)
        assert np.array_equal(start, keep)


# ---- prediction ---------------------------------------------------------------------------------

@pytest.mark.parametrize("d", lr.PREDICT_D)
def test_predict_matches_long_double(d):
    X, w = lr.predict_inputs(d)
    for b in lr.INTERCEPTS:
        s = ref.predict(X, w, b, threshold=None)
        sl = lr.predict(X, w, b, threshold=None)
        assert np.max(np.abs(s.astype(lr.LD) - sl)) <= PREDICT_ABS
        m = ref.svm_predict(X, w, b, threshold=None)
        ml = lr.svm_predict(X, w, b, threshold=None)
        assert np.max(np.abs(m.astype(lr.LD) - ml)) <= PREDICT_ABS
        safe = np.abs(sl - 0.5) > 1e-9
        assert safe.mean() >= 0.99
        assert np.array_equal(ref.predict(X, w, b)[safe], lr.predict(X, w, b)[safe])
        safe = np.abs(ml) > 1e-9
        assert safe.mean() >= 0.99
        assert np.array_equal(ref.svm_predict(X, w, b)[safe], lr.svm_predict(X, w, b)[safe])


def test_predict_saturates():
    """Margins of +-800: exp overflows to Inf (or underflows to 0) and the score is exactly 0.0 or
    1.0 in float64; in long double it is within 1e-300 of that."""
    X, w = lr.saturating_inputs(64)
    with np.errstate(over="ignore"):
        s = ref.predict(X, w, threshold=None)
    m = lr.svm_predict(X, w, threshold=None)
    assert float(m.max()) > 700 and float(m.min()) < -700
    big = np.asarray(m > 700) | np.asarray(m < -700)
    assert np.array_equal(s[big], np.asarray(m > 0, dtype=np.float64)[big])
    assert np.max(np.abs(s.astype(lr.LD) - lr.predict(X, w, threshold=None))) <= PREDICT_ABS


def test_predict_nan_row():
    X, w = lr.predict_inputs(65)
    Xp = lr.poisoned(X, 2, 64, np.nan)
    for fn, fl in ((ref.predict, lr.predict), (ref.svm_predict, lr.svm_predict)):
        s, sl = fn(Xp, w, threshold=None), fl(Xp, w, threshold=None)
        assert np.isnan(s[2]) and np.isnan(sl[2])
        assert fn(Xp, w)[2] == 0.0 and fl(Xp, w)[2] == 0.0          # NaN > t is false
        clean = np.arange(len(s)) != 2
        assert np.array_equal(s[clean], fn(X, w, threshold=None)[clean])


# ---- non-finite feature rows ----------------------------------------------------------------------

def parent_hinge_train(X, y, num_iterations, step_size, reg_param, convergence_tol=0.001):
    """The hinge loop as this oracle stated it before it skipped rows: every row multiplied,
    mult = 0.0 for the rows outside the hinge (0 * NaN = NaN)."""
    import math
    w = np.zeros(X.shape[1])
    prev, done = None, 0
    for i in range(1, num_iterations + 1):
        s_lab = 2.0 * y - 1.0
        mult = np.where(1.0 > s_lab * (X @ w), -s_lab, 0.0)
        grad = (mult[:, None] * X).sum(axis=0) / len(y)
        step = step_size / math.sqrt(i)
        w = w * (1.0 - step * reg_param)
        w = w - step * grad
        done = i
        if prev is not None and np.linalg.norm(prev - w) < convergence_tol * max(
                np.linalg.norm(w), 1.0):
            break
        prev = w.copy()
    return w, done


@pytest.mark.parametrize("n,d,reg", [(37, 48, 0.0), (300, 1, 0.01), (2100, 129, 0.01)])
def test_hinge_row_skipping_is_bit_neutral_on_finite_inputs(n, d, reg):
    X, y = lr.rows(n, d, 1000 * d + n)
    w, it = ref.sgd_train(X, y, 100, 1.0, reg, gradient="hinge")
    wp, itp = parent_hinge_train(X, y, 100, 1.0, reg)
    assert it == itp
    assert w.tobytes() == wp.tobytes()


@pytest.mark.parametrize("poison", list(lr.POISONS))
@pytest.mark.parametrize("d", lr.POISON_D)
@pytest.mark.parametrize("n", lr.POISON_N)
def test_non_finite_row_hinge(n, d, poison):
    """One NaN entry: the row is skipped in every iteration and the weights are finite.  One +-Inf
    entry meets the zero initial weights (margin 0 * Inf = NaN) and is skipped in iteration 1; once
    its weight is nonzero the margin is +-Inf and the row is inside or outside the hinge like any
    other.  The oracle equals the long-double reference either way."""
    X, y = lr.rows(n, d, 1000 * d + n)
    for r, f in lr.poison_places(n, d):
        Xp = lr.poisoned(X, r, f, lr.POISONS[poison])
        with np.errstate(invalid="ignore"):
            w, it = ref.sgd_train(Xp, y, 100, 1.0, 0.01, gradient="hinge")
            ld = lr.sgd_train(Xp, y, 100, 1.0, 0.01, gradient="hinge")
        wl = ld.weights.astype(np.float64)
        assert it == ld.iterations, (r, f)
        assert np.array_equal(lr.classes(w), lr.classes(wl)), (r, f)
        fin = lr.classes(wl) == 0
        if poison == "nan":
            assert fin.all(), (r, f)
        # over the finite differences and margins (all of them through a NaN entry)
        assert ld.conv_margin >= CONV_MARGIN and ld.hinge_gap >= HINGE_GAP, (r, f)
        assert norm(w[fin] - wl[fin]) <= ORACLE_REL * norm(wl[fin]), (r, f)
    # the first iteration alone (zero weights): every poison is skipped
    with np.errstate(invalid="ignore"):
        w1, _ = ref.sgd_train(Xp, y, 1, 1.0, 0.01, gradient="hinge")
    assert np.isfinite(w1).all()


@pytest.mark.parametrize("poison", list(lr.POISONS))
def test_non_finite_row_logistic(poison):
    """LogisticGradient multiplies every row: a NaN margin makes the multiplier NaN and with it
    every feature the row touches (all of them: no entry of these rows is zero)."""
    n, d = 37, 48
    X, y = lr.rows(n, d, 1000 * d + n)
    for r, f in lr.poison_places(n, d):
        Xp = lr.poisoned(X, r, f, lr.POISONS[poison])
        with np.errstate(invalid="ignore", over="ignore"):
            w, it = ref.sgd_train(Xp, y, 100, 1.0, 0.01)
            ld = lr.sgd_train(Xp, y, 100, 1.0, 0.01)
        assert it == ld.iterations == 100
        assert np.isnan(w).all() and np.isnan(ld.weights.astype(np.float64)).all()
