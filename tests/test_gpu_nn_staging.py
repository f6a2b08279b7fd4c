"""The `mem` flag of the eegfx_nn_* entries has the property tests/test_gpu_mem_staging.py states
for the other classifier and flow entries: host arrays are staged through the context's buffers,
device tensors are used in place, and the same kernels read the same bytes in the same order
either way.  So every comparison is bit for bit: host against device, a call among other entries'
calls on one context against the call alone on a fresh one, and a context's results before and
after another context's life."""
import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import classification as clf
from test_gpu_mem_staging import device, rows, same_bits

pytestmark = pytest.mark.gpu

N, D = 65, 3  # one row past a tile, a feature tail
SMALL = clf.NnModel(d=D, widths=(4, 2), activations=("tanh", "softmax"),
                    loss="negativeloglikelihood", updater="adam", num_iterations=4)
LARGE = clf.NnModel(d=48, widths=(16, 2), activations=("relu", "sigmoid"), loss="xent",
                    updater="nesterovs", num_iterations=3)


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


def stats(c, scores, labels):
    s = clf.nn_statistics(c, scores, labels)
    return np.array(s.as_tuple()), np.array([s.MSE, s.class1sum, s.class2sum])


def scores_and_labels(n, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 2, size=n).astype(np.float64)
    return np.clip(labels + 0.4 * rng.standard_normal(n), -0.7, 1.7), labels


def host_device_cases():
    X, y = rows(N, D, 1)
    s, a = scores_and_labels(300, 2)
    p = clf.nn_init_params(SMALL)
    return {
        "nn_train": (lambda c, X, y: clf.nn_train(c, X, y, SMALL), (X, y)),
        "nn_predict": (lambda c, X: clf.nn_predict(c, X, SMALL, p), (X,)),
        "nn_statistics": (stats, (s, a)),
    }


HOST_DEVICE = host_device_cases()


@pytest.mark.parametrize("name", sorted(HOST_DEVICE))
def test_host_equals_device(ctx, name):
    call, arrays = HOST_DEVICE[name]
    same_bits(call(ctx, *[device(a) for a in arrays]), call(ctx, *arrays))


def test_interleaved_entries_equal_each_alone(ctx):
    """Host-memory calls of the nn entries among the entries whose staging buffers they share
    (rows_x, row_vals), sizes small -> large -> small: each result equals that of the same call
    alone on a fresh context."""
    Xs, ys = rows(N, D, 11)
    Xl, yl = rows(1000, 48, 12)
    Xp, _ = rows(N, D, 13)
    s, a = scores_and_labels(300, 14)
    sl, al = scores_and_labels(5000, 15)
    ps, pl = clf.nn_init_params(SMALL), clf.nn_init_params(LARGE)
    steps = [
        lambda c: clf.nn_train(c, Xs, ys, SMALL),
        lambda c: clf.sgd_train(c, Xl, yl, 5),
        lambda c: clf.nn_train(c, Xl, yl, LARGE),
        lambda c: stats(c, s, a),
        lambda c: clf.nn_predict(c, Xp, SMALL, ps),
        lambda c: clf.dtree_train(c, Xl, yl),
        lambda c: clf.nn_predict(c, Xl, LARGE, pl),
        lambda c: stats(c, sl, al),
        lambda c: clf.nn_train(c, Xs, ys, SMALL),
        lambda c: stats(c, s, a),
    ]
    together = fx.Context(0)
    try:
        got = [step(together) for step in steps]
    finally:
        together.close()
    for step, g in zip(steps, got):
        alone = fx.Context(0)
        try:
            same_bits(g, step(alone))
        finally:
            alone.close()


def test_context_life_leaves_another_context_working(ctx):
    """A context that ran every nn entry once is destroyed (its nn buffers released with the
    rest) while another stays open: the open one computes what it computed before."""
    X, y = rows(N, D, 21)
    before = clf.nn_train(ctx, X, y, SMALL)
    other = fx.Context(0)
    try:
        p, _ = clf.nn_train(other, X, y, SMALL)
        stats(other, clf.nn_predict(other, X, SMALL, p), y)
        clf.nn_train(other, device(X), device(y), SMALL)
    finally:
        other.close()
    same_bits(clf.nn_train(ctx, X, y, SMALL), before)
