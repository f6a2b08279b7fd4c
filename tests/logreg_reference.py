"""Long-double reference of the classifier loop, and the cases shared by test_logreg_reference.py
(CPU: pins oracle/mllib_logreg.py against this reference on them and checks their conditioning)
and test_gpu_logreg_shapes.py (GPU: compares the device with the oracle on them).  Not a test
module.

The loop is MLlib 1.6.2 GradientDescent.runMiniBatchSGD written row-wise from the definitions, in
np.longdouble (x87 80-bit where the platform has it, eps 1.08e-19):

  margin      m = X @ w
  logistic    LogisticGradient (binary): multiplier 1 / (1 + exp(-m)) - y, gradient += multiplier x
  hinge       HingeGradient: s = 2 y - 1; the rows with 1.0 > s m (a boolean mask: a NaN comparison
              is false, the row is skipped as MLlib skips its axpy) have their -s x summed; no
              other row is ever multiplied
  gradient    / sample size
  update      SquaredL2Updater: w = w (1 - step_i reg) - step_i g, step_i = step / sqrt(i)
  converged   from the second updated iterate: ||w_prev - w|| < tol max(||w||, 1)
  mini-batch  rows_of_iteration(i) names iteration i's rows (feed it oracle.mllib_logreg.
              sample_rows, which test_spark_sample.py pins); an empty sample skips the update and
              the convergence test

It shares no expression with oracle/mllib_logreg.py, which states the same loop in float64.
"""
from collections import namedtuple

import numpy as np

LD = np.longdouble

Run = namedtuple("Run", "weights iterations conv_margin hinge_gap")
Run.__doc__ = """weights (long double), iterations run, and the run's two conditioning numbers:
conv_margin  min over the convergence tests made of |diff / threshold - 1| (inf if none was made):
             how far the closest test was from flipping;
hinge_gap    min over all rows used and all iterations of |1 - s m| (inf for logistic): how far
             the closest row was from changing side of the hinge."""


def sgd_train(X, y, num_iterations=100, step_size=1.0, reg_param=0.0, convergence_tol=0.001,
              initial=None, gradient="logistic", rows_of_iteration=None):
    X = np.asarray(X, dtype=LD)
    y = np.asarray(y, dtype=LD)
    n, d = X.shape
    w = np.zeros(d, dtype=LD) if initial is None else np.array(initial, dtype=LD)
    one = LD(1)
    prev = None
    done = 0
    conv_margin = np.inf
    hinge_gap = np.inf
    for i in range(1, num_iterations + 1):
        done = i
        Xs, ys = X, y
        if rows_of_iteration is not None:
            rows = list(rows_of_iteration(i))
            if not rows:
                continue
            Xs, ys = X[rows], y[rows]
        m = Xs @ w
        if gradient == "hinge":
            s = 2 * ys - one
            sm = s * m
            gaps = np.abs(one - sm)
            gaps = gaps[np.isfinite(gaps)]
            if gaps.size:
                hinge_gap = min(hinge_gap, float(gaps.min()))
            sel = one > sm
            g = (-s[sel][:, None] * Xs[sel]).sum(axis=0)
        else:
            mult = one / (one + np.exp(-m)) - ys
            g = (mult[:, None] * Xs).sum(axis=0)
        g = g / LD(len(ys))
        step = LD(step_size) / np.sqrt(LD(i))
        w = w * (one - step * LD(reg_param)) - step * g
        if prev is not None:
            diff = np.sqrt(((prev - w) ** 2).sum())
            threshold = LD(convergence_tol) * max(np.sqrt((w ** 2).sum()), one)
            if threshold > 0 and np.isfinite(diff):
                conv_margin = min(conv_margin, float(abs(diff / threshold - one)))
            if diff < threshold:
                break
        prev = w.copy()
    return Run(w, done, conv_margin, hinge_gap)


def predict(X, w, intercept=0.0, threshold=0.5):
    """LogisticRegressionModel.predict: the score 1 / (1 + exp(-(w.x + b))), or score > threshold."""
    m = np.asarray(X, dtype=LD) @ np.asarray(w, dtype=LD) + LD(intercept)
    score = LD(1) / (LD(1) + np.exp(-m))
    return score if threshold is None else (score > LD(threshold)).astype(np.float64)


def svm_predict(X, w, intercept=0.0, threshold=0.0):
    """SVMModel.predict: the margin w.x + b, or margin > threshold."""
    m = np.asarray(X, dtype=LD) @ np.asarray(w, dtype=LD) + LD(intercept)
    return m if threshold is None else (m > LD(threshold)).astype(np.float64)


# ---- the cases --------------------------------------------------------------------------------

def rows(n, d, seed):
    """The generator of test_gpu_logreg.py: unit-norm rows with a planted separating direction."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    w0 = rng.standard_normal(d)
    y = (X @ w0 + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    return X, y


Case = namedtuple("Case", "n d gradient iters step reg fraction parts start seed",
                  defaults=(100, 1.0, 0.01, 1.0, 1, False, None))
Case.__doc__ = """One training run: rows(n, d, seed or 1000 d + n); start: a random nonzero
initial weight vector (initial_weights()) instead of zeros."""

GRADIENTS = ("logistic", "hinge")

# every FPL instance of the narrow gradient kernel (d <= 128) at its first and last d -- 65..112
# leave whole feature slots of FPL 8 past d -- and the update kernel's group counts 256, 128, 3, 2
NARROW_D = (1, 2, 16, 17, 32, 33, 49, 64, 65, 85, 86, 100, 112, 113, 128)
# every KD instance of the wide gradient kernel at its first and last d
WIDE_ND = ((2100, 129), (2100, 256), (2100, 257), (600, 513), (600, 1024))
# less than one quad of rows, a partial 16-row group, one workgroup and the step to two
SMALL_N = (1, 3, 4, 5, 63, 64, 65)
# the narrow kernel's grid covers 32768 rows per pass: one pass exactly, a second pass of one row,
# a partial second pass
LARGE_N = (32768, 32769, 40000)
LARGE_ITERS = 30
MAX_D = 1024

# Seeds other than 1000 d + n, and parameters other than the defaults: where the default case sits
# on a rounding (conv_margin < 1e-4 or hinge_gap < 1e-6 in the long-double run).
#   n = 1 hinge at step 1.0: the first update makes w = s x of the one unit-norm row, so the second
#   iteration's margin is |x|^2 = 1.0 up to its rounding (hinge_gap 0 to 2e-16).
_STEP = {(1, d, "hinge"): 0.3 for d in (1, 20, 48, 129)}
_SEED = {}


def _case(n, d, g, **kw):
    kw.setdefault("step", _STEP.get((n, d, g), 1.0))
    kw.setdefault("seed", _SEED.get((n, d, g)))
    return Case(n, d, g, **kw)


BUCKET_CASES = [_case(n, d, g) for g in GRADIENTS
                for n, d in [(300, d) for d in NARROW_D] + list(WIDE_ND)]
ROW_CASES = ([_case(n, d, g) for g in GRADIENTS for d in (48, 20) for n in SMALL_N]
             + [_case(n, d, g, iters=LARGE_ITERS) for g in GRADIENTS for d in (48, 20)
                for n in LARGE_N]
             + [_case(n, 129, g) for g in GRADIENTS for n in (1, 4, 2049)])
# n = 40 at f = 0.03 has iterations whose sample is empty (d = 20, not the 48 of
# test_gpu_logreg.py's)
EMPTY_SAMPLE_ND = (40, 20)
MINI_BATCH_ND = ((2100, 129, 100), (600, 1024, 100), (40000, 20, LARGE_ITERS), (300, 100, 100),
                 EMPTY_SAMPLE_ND + (100,))
MINI_BATCH_CASES = [_case(n, d, "logistic", iters=it, fraction=f, parts=4)
                    for n, d, it in MINI_BATCH_ND for f in (0.03, 0.5)]
# the oracle alone (the device's hinge loop is full-batch only)
MINI_BATCH_HINGE_CASES = [c._replace(gradient="hinge") for c in MINI_BATCH_CASES]
START_CASES = [_case(n, d, g, start=True) for g in GRADIENTS for n, d in ((300, 48), (2100, 257))]
DETERMINISM_CASES = [_case(n, d, g) for g in GRADIENTS for n, d in ((5000, 48), (2100, 257))]

GPU_CASES = BUCKET_CASES + ROW_CASES + MINI_BATCH_CASES + START_CASES + DETERMINISM_CASES
ALL_CASES = GPU_CASES + MINI_BATCH_HINGE_CASES


def case_id(c):
    s = f"{c.gradient}-n{c.n}-d{c.d}"
    if c.fraction < 1.0:
        s += f"-f{c.fraction}"
    if c.start:
        s += "-start"
    return s


def case_rows(c):
    return rows(c.n, c.d, 1000 * c.d + c.n if c.seed is None else c.seed)


def initial_weights(d):
    """A nonzero start of about the size of a trained vector."""
    return np.random.default_rng(77 + d).standard_normal(d) * 0.5


def case_start(c):
    return initial_weights(c.d) if c.start else None


# ---- non-finite feature rows ------------------------------------------------------------------
POISONS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
POISON_N = (37, 257)         # one partial workgroup; 5 workgroups with a 1-row tail
POISON_D = (48, 100, 257)    # narrow kernel without and with slots past d, wide kernel


def poison_places(n, d):
    """(row, column) of the poisoned entry: the first, a middle and the last row -- row n - 1 is
    the one the hinge instance re-reads for rows past n -- each with the first, a middle and the
    last feature -- feature d - 1 is the one it re-reads for slots past d."""
    return [(r, f) for r in (0, n // 2, n - 1) for f in (0, d // 2, d - 1)]


def poisoned(X, r, f, value):
    Xp = X.copy()
    Xp[r, f] = value
    return Xp


def classes(w):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf per entry."""
    w = np.asarray(w, dtype=np.float64)
    return np.where(np.isnan(w), 1, np.where(w == np.inf, 2, np.where(w == -np.inf, 3, 0)))


# ---- prediction ---------------------------------------------------------------------------------
# every KD instance of the predict kernel at its first and last d
PREDICT_D = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
# less than one workgroup (4 rows), one, one and a row, many and a row
PREDICT_N = (1, 3, 4, 5, 4097)
INTERCEPTS = (0.0, 0.25, -3.0)


def predict_inputs(d):
    """(X, w): max(PREDICT_N) unit-norm rows (the tests take the first n) and a weight vector that
    spreads the margins over about +-6."""
    X, _ = rows(max(PREDICT_N), d, 5000 + d)
    w = 2.0 * np.random.default_rng(6000 + d).standard_normal(d)
    return X, w


def saturating_inputs(d):
    """(X, w) with the weights along +-the rows' own direction, scaled so that the margins reach
    +-800: past exp's float64 range (709.78), where the score is exactly 0.0 or 1.0."""
    X, _ = rows(9, d, 7000 + d)
    w = 800.0 * (X[0] - X[1]) / (1.0 - X[0] @ X[1])
    return X, w
