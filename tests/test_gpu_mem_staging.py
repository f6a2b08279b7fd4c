"""The `mem` flag of the classifier, flow and planning entries: host arrays are staged through the
context's buffers (csrc/ctx.h stage_in / dev_out / copy_back), device tensors are used in place,
and the same kernels read the same bytes in the same order either way.  So every comparison here
is bit for bit: host against device, a call among other entries' calls on one context against the
call alone on a fresh one, and a context's results before and after another context's life."""
import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import classification as clf
from eeg_dataanalysispackage_amd.pipeline import gather_rows
from conftest import INFO_TRAIN

pytestmark = pytest.mark.gpu

N, D = 65, 3  # one row past a wave, a feature tail


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


def rows(n, d, seed):
    """Feature rows and 0/1 labels that a plane separates but for some noise."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = (X @ rng.standard_normal(d) + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    return X, y


def marker_data(n, seed):
    rng = np.random.default_rng(seed)
    n_frames = 10 * n + 5000
    pos = rng.integers(-50, n_frames + 300, size=n)  # some cuts leave the recording
    return pos, rng.integers(-1, 6, size=n).astype(np.int32), n_frames


def plan(ctx, pos, stim, n_frames):
    p, lab, balance = ctx.plan_markers(pos, stim, n_frames, 3, 0)
    return p, lab, balance, len(p)  # pos_out, label_out, balance, n_selected


def gather_data(n_src, d, m, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_src, size=m)
    idx[7] = idx[3]  # a repeated index
    return rng.standard_normal((n_src, d)), idx.astype(np.int64)


def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(v):
    """A result's bytes: of a numpy array (structured ones too), a device tensor or an integer."""
    if hasattr(v, "is_cuda"):
        v = v.cpu().numpy()
    return np.ascontiguousarray(v).reshape(-1).view(np.uint8)


def same_bits(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(raw(g), raw(w))


@pytest.fixture(scope="module")
def models(ctx):
    """Models for the predict cases, trained once from host rows."""
    X, y = rows(N, D, 1)
    Xw, yw = rows(1000, 48, 2)
    return dict(w=clf.sgd_train(ctx, X, y, 5)[0], svm_w=clf.svm_sgd_train(ctx, X, y, 5)[0],
                tree=clf.dtree_train(ctx, X, y),
                forest=clf.rforest_train(ctx, X, y, num_trees=3, feature_subset="sqrt",
                                         num_partitions=2),
                w48=clf.sgd_train(ctx, Xw, yw, 5)[0],
                forest48=clf.rforest_train(ctx, Xw, yw, num_trees=3, num_partitions=2))


# name -> (the call on (ctx, models, *arrays), the arrays): each array goes in once as numpy and
# once as a device tensor
def host_device_cases():
    X, y = rows(N, D, 1)
    src, idx = gather_data(65, D, 40, 3)
    pred = (np.arange(N) % 3 == 0).astype(np.float64)
    pos, stim, n_frames = marker_data(65, 4)
    return {
        "sgd_train": (lambda c, m, X, y: clf.sgd_train(c, X, y, 5), (X, y)),
        "sgd_train_mini_batch": (lambda c, m, X, y: clf.sgd_train(
            c, X, y, 5, mini_batch_fraction=0.5, num_partitions=3), (X, y)),
        "svm_sgd_train": (lambda c, m, X, y: clf.svm_sgd_train(c, X, y, 5), (X, y)),
        "predict": (lambda c, m, X: clf.predict(c, X, m["w"]), (X,)),
        "predict_scores": (lambda c, m, X: clf.predict(c, X, m["w"], threshold=None), (X,)),
        "svm_predict": (lambda c, m, X: clf.svm_predict(c, X, m["svm_w"]), (X,)),
        "svm_predict_margins": (lambda c, m, X: clf.svm_predict(c, X, m["svm_w"], threshold=None),
                                (X,)),
        "dtree_train": (lambda c, m, X, y: clf.dtree_train(c, X, y), (X, y)),
        "dtree_predict": (lambda c, m, X: clf.dtree_predict(c, X, m["tree"]), (X,)),
        "rforest_train": (lambda c, m, X, y: clf.rforest_train(
            c, X, y, num_trees=3, feature_subset="sqrt", num_partitions=2), (X, y)),
        "rforest_predict": (lambda c, m, X: clf.rforest_predict(c, X, *m["forest"]), (X,)),
        "gather_rows": (lambda c, m, src, idx: gather_rows(c, src, idx), (src, idx)),
        "confusion_counts": (lambda c, m, p, a: np.array(clf.confusion_counts(c, p, a)),
                             (pred, y)),
        "plan_markers_device": (lambda c, m, pos, stim: plan(c, pos, stim, n_frames), (pos, stim)),
    }


HOST_DEVICE = host_device_cases()


@pytest.mark.parametrize("name", sorted(HOST_DEVICE))
def test_host_equals_device(ctx, models, name):
    call, arrays = HOST_DEVICE[name]
    same_bits(call(ctx, models, *[device(a) for a in arrays]), call(ctx, models, *arrays))


def test_interleaved_entries_equal_each_alone(ctx, models):
    """Host-memory calls of the entries that share staging buffers, sizes small -> large -> small:
    a grow-only buffer is reallocated after another entry last used it and reused at a smaller
    size.  Each result equals that of the same call alone on a fresh context."""
    Xs, ys = rows(N, D, 11)
    Xl, yl = rows(1000, 48, 12)
    Xp, _ = rows(N, D, 13)
    Xf, _ = rows(1000, 48, 14)
    Xt, _ = rows(N, D, 15)
    Xw, yw = rows(1000, 48, 16)
    pos, stim, n_frames = marker_data(1000, 17)
    src, idx = gather_data(65, D, 40, 18)
    p, a = rows(300, 1, 19)[1], rows(300, 1, 20)[1]
    steps = [
        lambda c: plan(c, pos, stim, n_frames),
        lambda c: clf.sgd_train(c, Xs, ys, 5),
        lambda c: clf.dtree_train(c, Xl, yl),
        lambda c: clf.predict(c, Xp, models["w"]),
        lambda c: clf.rforest_predict(c, Xf, *models["forest48"]),
        lambda c: gather_rows(c, src, idx),
        lambda c: np.array(clf.confusion_counts(c, p, a)),
        lambda c: clf.dtree_predict(c, Xt, models["tree"]),
        lambda c: clf.sgd_train(c, Xw, yw, 5),
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


def test_context_life_leaves_another_context_working(ctx, models):
    """A context that ran every classifier and flow entry once is destroyed (every buffer of the
    context released) while another stays open: the open one computes what it computed before."""
    X, y = rows(N, D, 21)
    before = clf.sgd_train(ctx, X, y, 5)
    other = fx.Context(0)
    try:
        pos, stim, n_frames = marker_data(65, 22)
        plan(other, pos, stim, n_frames)
        w = clf.sgd_train(other, X, y, 5, mini_batch_fraction=0.5, num_partitions=3)[0]
        clf.predict(other, X, w)
        clf.svm_predict(other, X, clf.svm_sgd_train(other, X, y, 5)[0])
        clf.dtree_predict(other, X, clf.dtree_train(other, X, y))
        clf.rforest_predict(other, X, *clf.rforest_train(other, X, y, num_trees=3,
                                                         num_partitions=2))
        gather_rows(other, *gather_data(65, D, 40, 23))
        clf.confusion_counts(other, (np.arange(N) % 2).astype(np.float64), y)
        odp = fx.OffLineDataProvider([INFO_TRAIN], context=other)
        try:
            odp.loadData()
            odp.split(device=False, context=other)
        finally:
            odp.close()
    finally:
        other.close()
    same_bits(clf.sgd_train(ctx, X, y, 5), before)
