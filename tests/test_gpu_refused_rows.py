"""The device-side refusals of the classifiers and the train/test flow, with the offending row in
the later trips, unroll slots and workgroups of each kernel's capped grid-stride loop: a label that
is not 0.0 or 1.0 (lr_validate_kernel, dt_bin_kernel, confusion_kernel), a non-finite training
feature (dt_bin_kernel) and a gather index outside its source (gather_rows_kernel).

tests/refusal_cases.py names the rows and sizes;
tests/test_refusal_cases.py asserts off the GPU that each row falls where its case says.  Every
assertion is exact (an error code, a message, bits), but for the one clean SGD run per gradient,
held to oracle/mllib_logreg.py at test_gpu_logreg.py's bar."""
import numpy as np
import pytest
import torch

import dtree_reference as D
import refusal_cases as R
import rforest_reference as RF
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib, classification as clf
from eeg_dataanalysispackage_amd._lib import ptr
from oracle import mllib_logreg as ref
from test_gpu_dtree import same_tree
from test_gpu_logreg import close
from test_gpu_rforest import same_forest

pytestmark = pytest.mark.gpu

DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
BAD_LABELS_TEXT = "Input validation failed: labels must be 0.0 or 1.0"
FOREST = dict(num_trees=3, feature_subset="sqrt", num_partitions=2, seed=12345)
SENT = -1.2345e300
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def refused(code, text, call):
    with pytest.raises(fx.EegfxError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


# ---- the SGD trainers -----------------------------------------------------------------------------
TRAINERS = {"logistic": (clf.sgd_train, {}), "hinge": (clf.svm_sgd_train, {"gradient": "hinge"})}


@pytest.fixture(scope="module")
def sgd_rows():
    rng = np.random.default_rng(R.LR_N)
    X = rng.standard_normal((R.LR_N, 1))
    y = (X[:, 0] + 0.3 * rng.standard_normal(R.LR_N) > 0).astype(np.float64)
    return X, y


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("gradient", sorted(TRAINERS))
def test_sgd_label_in_every_trip_of_the_validation(ctx, sgd_rows, gradient, mem):
    train, kw = TRAINERS[gradient]
    X, y = sgd_rows
    y = y.copy()
    Xm, ym = (X, y) if mem == "host" else (cuda(X), cuda(y))
    for row in R.LR_ROWS:
        for bad in R.BAD_LABELS:
            good = float(y[row])
            ym[row] = bad
            refused(_lib.EEGFX_EINVAL, BAD_LABELS_TEXT, lambda: train(ctx, Xm, ym, 1, 1.0, 0.0))
            ym[row] = good
    w, it = train(ctx, Xm, ym, 1, 1.0, 0.0)
    wr, itr = ref.sgd_train(X, y, 1, 1.0, 0.0, **kw)
    assert it == itr == 1 and close(w, wr)


# ---- the tree and the forest ----------------------------------------------------------------------
def tree_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = (X @ rng.standard_normal(d) + 0.5 * rng.standard_normal(n) > 0).astype(np.float64)
    return X, y


def grow(ctx, kind, X, y, **kw):
    if kind == "dtree":
        return clf.dtree_train(ctx, X, y, max_depth=2, max_bins=8, **kw)
    return clf.rforest_train(ctx, X, y, max_depth=2, max_bins=8, **FOREST, **kw)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kind", ["dtree", "rforest"])
def test_tree_rows_at_both_ends_of_the_binning(ctx, kind, mem):
    n, d = R.TREE_N, R.TREE_D
    X, y = tree_rows(n, d, 51)
    put = (lambda a: a) if mem == "host" else cuda
    for row in (0, n - 1):
        for bad in R.BAD_LABELS:
            yb = y.copy()
            yb[row] = bad
            refused(_lib.EEGFX_EINVAL, BAD_LABELS_TEXT, lambda: grow(ctx, kind, put(X), put(yb)))
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[n - 1, d - 1] = bad
        refused(_lib.EEGFX_EINVAL, "not finite", lambda: grow(ctx, kind, put(Xb), put(y)))
    grow(ctx, kind, put(X), put(y))     # and the clean rows train


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kind", ["dtree", "rforest"])
def test_tree_non_finite_value_in_the_last_unsampled_row(ctx, kind, mem):
    """n above Spark's sample bound: the thresholds come from the sampled rows, which the host
    checks; a row outside the sample meets dt_bin_kernel alone, here in a later trip."""
    n, d = R.TREE_SAMPLED_N, R.TREE_SAMPLED_D
    X, y = tree_rows(n, d, 29)
    kept = clf.spark_sample(n, 10000 / n, 1, 0)
    last = int(np.setdiff1d(np.arange(n), kept)[-1])
    assert R.bin_place(last, d - 1, n, d).trip >= 1
    put = (lambda a: a) if mem == "host" else cuda
    for bad in (np.nan, -np.inf):
        Xb = X.copy()
        Xb[last, d - 1] = bad
        refused(_lib.EEGFX_EINVAL, "not finite",
                lambda: grow(ctx, kind, put(Xb), put(y), split_seed=0))
    got = grow(ctx, kind, put(X), put(y), split_seed=0)
    if kind == "dtree":
        same_tree(got, D.train(X, y, "gini", max_depth=2, max_bins=8, sample_rows=kept))
    else:
        same_forest(got, RF.train(X, y, "gini", max_depth=2, max_bins=8, sample_rows=kept,
                                  num_trees=3, feature_subset="sqrt", seed=12345, num_partitions=2,
                                  weights=RF.bag(n, 3, 2, 12345)))


# ---- negative zero --------------------------------------------------------------------------------
def with_negative_zeros(y):
    z = y.copy()
    z[y == 0.0] = -0.0
    assert np.signbit(z).any() and np.array_equal(z, y)
    return z


@pytest.mark.parametrize("gradient", sorted(TRAINERS))
def test_negative_zero_label_is_class_0_in_the_sgd_trainers(ctx, gradient):
    """DataValidators.binaryLabelValidator compares numerically (label == 0 || label == 1), and
    so do the kernels: -0.0 passes, and the gradient's arithmetic cannot tell it from +0.0."""
    train, kw = TRAINERS[gradient]
    rng = np.random.default_rng(7)
    X = rng.standard_normal((300, 5))
    y = (X[:, 0] > 0).astype(np.float64)
    z = with_negative_zeros(y)
    w, it = train(ctx, X, y, 20, 1.0, 0.01)
    for Xm, zm in ((X, z), (cuda(X), cuda(z))):
        wz, itz = train(ctx, Xm, zm, 20, 1.0, 0.01)
        assert itz == it and wz.tobytes() == w.tobytes()
    wr, itr = ref.sgd_train(X, z, 20, 1.0, 0.01, **kw)
    assert itr == it and close(w, wr)


@pytest.mark.parametrize("kind", ["dtree", "rforest"])
def test_negative_zero_label_is_class_0_in_the_trees(ctx, kind):
    X, y = tree_rows(R.TREE_N, R.TREE_D, 53)
    z = with_negative_zeros(y)
    if kind == "dtree":
        want = D.train(X, z, "gini", max_depth=2, max_bins=8)
        for Xm, zm in ((X, z), (cuda(X), cuda(z)), (X, y)):
            same_tree(grow(ctx, kind, Xm, zm), want)
    else:
        want = RF.train(X, z, "gini", max_depth=2, max_bins=8, num_trees=3, feature_subset="sqrt",
                        seed=12345, num_partitions=2, weights=RF.bag(R.TREE_N, 3, 2, 12345))
        for Xm, zm in ((X, z), (cuda(X), cuda(z)), (X, y)):
            same_forest(grow(ctx, kind, Xm, zm), want)


def test_negative_zero_label_is_class_0_in_the_confusion_counts(ctx):
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 2, size=300).astype(np.float64)
    pred = rng.integers(0, 2, size=300).astype(np.float64)
    z = with_negative_zeros(labels)
    want = clf.reference_statistics(pred, z).as_tuple()
    assert want == clf.reference_statistics(pred, labels).as_tuple()
    for mem in (DEV, HOST):
        assert counts(ctx, pred, z, mem) == (_lib.EEGFX_OK, want)
    # -0.0 alone is one class, as +0.0 alone
    assert counts(ctx, pred, np.full(300, -0.0), DEV)[0] == _lib.EEGFX_ERANGE
    with pytest.raises(IndexError):
        clf.reference_statistics(pred, np.full(300, -0.0))


# ---- the confusion counts -------------------------------------------------------------------------
def counts(ctx, pred, labels, mem):
    """eegfx_confusion_counts on host arrays or device tensors: (status, (tp, tn, fp, fn))."""
    out = np.full(4, -9, dtype=np.int64)
    if mem == DEV and not torch.is_tensor(pred):
        pred, labels = cuda(pred), cuda(labels)
    if mem == DEV:
        torch.cuda.synchronize()
    rc = fx.lib().eegfx_confusion_counts(ctx.handle, ptr(pred), ptr(labels), int(pred.shape[0]),
                                         ptr(out), mem)
    return rc, tuple(int(v) for v in out)


def vectorised_counts(pred, labels):
    """classification.reference_statistics for labels that hold both classes, as boolean sums."""
    a1, a0, p1, p0 = labels == 1.0, labels == 0.0, pred == 1.0, pred == 0.0
    return (int((a1 & p1).sum()), int((a0 & p0).sum()), int((a1 & p0).sum()), int((a0 & p1).sum()))


def test_the_vectorised_counts_are_reference_statistics():
    rng = np.random.default_rng(10)
    n = R.CONFUSION_SMALL_N
    labels = rng.integers(0, 2, size=n).astype(np.float64)
    pred = rng.integers(0, 2, size=n).astype(np.float64)
    pred[rng.integers(0, n, size=100)] = np.array([np.nan, 0.5, 2.0, -0.0])[np.arange(100) % 4]
    want = clf.reference_statistics(pred, labels).as_tuple()
    assert vectorised_counts(pred, labels) == want and sum(want) < n


@pytest.mark.parametrize("mem", [DEV, HOST])
def test_confusion_label_in_every_unroll_slot(ctx, mem):
    n = R.CONFUSION_SMALL_N
    rng = np.random.default_rng(11)
    pred = rng.integers(0, 2, size=n).astype(np.float64)
    for row in R.CONFUSION_SMALL_ROWS:
        for bad in R.BAD_LABELS:
            labels = np.resize([0.0, 1.0], n)
            labels[row] = bad
            rc, _ = counts(ctx, pred, labels, mem)
            assert rc == _lib.EEGFX_EINVAL, (row, bad)
            assert BAD_LABELS_TEXT in fx.lib().eegfx_last_error().decode()
        # the only row of class 1: its presence bit and its cell come from this slot alone
        labels = np.zeros(n)
        labels[row] = 1.0
        assert counts(ctx, pred, labels, mem) == (_lib.EEGFX_OK, vectorised_counts(pred, labels)), row
        labels = np.ones(n)
        labels[row] = 0.0
        assert counts(ctx, pred, labels, mem) == (_lib.EEGFX_OK, vectorised_counts(pred, labels)), row


def test_confusion_label_in_the_second_trip(ctx):
    n = R.CONFUSION_BIG_N
    rng = np.random.default_rng(12)
    pred = torch.from_numpy(rng.integers(0, 2, size=n).astype(np.float64)).cuda()
    labels = torch.zeros(n, dtype=torch.float64, device="cuda")
    rc, _ = counts(ctx, pred, labels, DEV)
    assert rc == _lib.EEGFX_ERANGE                   # no class-1 row
    assert "one class" in fx.lib().eegfx_last_error().decode()
    for bad in R.BAD_LABELS:
        labels[n - 1] = bad
        rc, _ = counts(ctx, pred, labels, DEV)
        assert rc == _lib.EEGFX_EINVAL, bad
        assert BAD_LABELS_TEXT in fx.lib().eegfx_last_error().decode()
    labels[n - 1] = 1.0
    p = pred.cpu().numpy()
    want = vectorised_counts(p, labels.cpu().numpy())
    assert sum(want) == n and want[0] + want[2] == 1
    assert counts(ctx, pred, labels, DEV) == (_lib.EEGFX_OK, want)


# ---- the gather -----------------------------------------------------------------------------------
def aligned(count, dtype, fill=None):
    """A device buffer whose first element lies on a 16-byte boundary."""
    buf = torch.empty(count + 2, dtype=dtype, device="cuda")
    buf = buf[(-buf.data_ptr() % 16) // buf.element_size():][:count]
    assert buf.data_ptr() % 16 == 0
    if fill is not None:
        buf.fill_(fill)
    return buf


@pytest.mark.parametrize("d", sorted(R.GATHER_SHAPES))
def test_gather_bad_index_in_the_second_trip(ctx, d):
    m, n_src = R.GATHER_SHAPES[d], R.GATHER_N_SRC
    rng = np.random.default_rng(d)
    src = aligned(n_src * d, torch.float64)
    src.copy_(torch.from_numpy(rng.standard_normal(n_src * d)))
    src[3] = -0.0
    src[7] = float("nan")
    good = torch.from_numpy(rng.integers(0, n_src, size=m)).cuda()
    first, last = R.gather_bad_rows(m)
    whole = aligned(m * d + 2 * GUARD, torch.float64)
    dst = whole[GUARD:GUARD + m * d]
    assert dst.data_ptr() % 16 == 0
    for rows, named in (((first, last), first), ((R.GATHER_EARLY_ROW, first, last),
                                                  R.GATHER_EARLY_ROW), ((last,), last)):
        idx = good.clone()
        idx[list(rows)] = torch.tensor([n_src, -1, 2 ** 40][:len(rows)], device="cuda")
        whole.fill_(SENT)
        torch.cuda.synchronize()
        rc = fx.lib().eegfx_gather_rows(ctx.handle, ptr(src), n_src, d, ptr(idx), m, ptr(dst), DEV)
        assert rc == _lib.EEGFX_ERANGE, rows
        assert f"idx[{named}] " in fx.lib().eegfx_last_error().decode(), rows
        ok = torch.ones(m, dtype=torch.bool, device="cuda")
        ok[list(rows)] = False
        got = dst.view(m, d)
        want = src.view(n_src, d)[good]
        assert torch.equal(got[ok].view(torch.int64), want[ok].view(torch.int64)), rows
        assert bool((got[~ok] == SENT).all()), rows             # nothing copied for a bad index
        assert bool((whole[:GUARD] == SENT).all()) and bool((whole[GUARD + m * d:] == SENT).all())
    whole.fill_(SENT)
    torch.cuda.synchronize()
    rc = fx.lib().eegfx_gather_rows(ctx.handle, ptr(src), n_src, d, ptr(good), m, ptr(dst), DEV)
    assert rc == _lib.EEGFX_OK
    assert torch.equal(dst.view(m, d).view(torch.int64),
                       src.view(n_src, d)[good].view(torch.int64))
