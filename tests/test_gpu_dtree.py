"""train_clf=dt on the GPU (csrc/dtree.hip, eegfx_dtree_*) against the Python restatement of MLlib
1.6.2 DecisionTree (tests/dtree_reference.py, pinned by tests/test_dtree_reference.py).  The
statistics are integer counts and the gains the same IEEE operations, so the bar is equality: every
node's id, feature, children, predict, impurity and gain, and its threshold by ==.  Parity with
Spark itself is unpinned (no fixture holds a trained tree)."""
from ctypes import byref, c_int32

import numpy as np
import pytest
import torch

import dtree_reference as R
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd import classification as clf
from conftest import INFO_TRAIN

pytestmark = pytest.mark.gpu
KINDS = ("gini", "entropy")


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0, numerics="exact")
    yield c
    c.close()


def rows(n, d, seed):
    """Gaussian features, labels from a noisy linear rule."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = (X @ rng.standard_normal(d) + 0.5 * rng.standard_normal(n) > 0).astype(np.float64)
    return X, y


def probes(X, seed):
    """Rows to predict on: fresh ones (77: no multiple of 64), and some holding NaN and +-Inf."""
    rng = np.random.default_rng(seed)
    d = X.shape[1]
    fresh = rng.standard_normal((77, d)) * 1.5
    odd = rng.standard_normal((9, d))
    for i, v in enumerate((np.nan, np.inf, -np.inf) * 3):
        odd[i, rng.integers(0, d)] = v
    odd[8, :] = np.nan
    return np.concatenate([fresh, odd])


def same_tree(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k in ("id", "feature", "left", "right", "predict", "impurity", "gain"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (k, bad[:4], got[k][bad[:4]], want[k][bad[:4]])
    assert np.all(got["threshold"] == want["threshold"])


def check(ctx, X, y, sample_rows=None, split_seed=0, **params):
    """Both impurities: the device's tree is the restatement's, and so are its predictions on the
    training rows, fresh rows, rows with NaN / Inf, and no rows at all."""
    P = probes(X, 5)
    trees = []
    for kind in KINDS:
        got = clf.dtree_train(ctx, X, y, impurity=kind, split_seed=split_seed, **params)
        want = R.train(X, y, kind, sample_rows=sample_rows, **params)
        same_tree(got, want)
        for Z in (X, P, P[:0]):
            assert np.array_equal(clf.dtree_predict(ctx, Z, got), R.predict(want, Z))
        trees.append(got)
    return trees


@pytest.mark.parametrize("d", [1, 3, 48, 65, 130])
@pytest.mark.parametrize("n", [2, 7, 63, 64, 65, 257, 1000])
def test_tree_matches_restatement(ctx, n, d):
    X, y = rows(n, d, 1000 * n + d)
    trees = check(ctx, X, y)
    if n >= 257:
        assert len(trees[0]) > 3  # the shapes grow real trees


@pytest.mark.parametrize("n,d,max_bins", [(257, 3, 2), (257, 3, 4), (300, 48, 32), (257, 3, 256),
                                          (1000, 130, 256), (63, 5, 256), (20, 3, 32)])
def test_bin_counts(ctx, n, d, max_bins):
    # 256 bins of 130 features do not fit the histogram kernel's LDS: the global-atomic form;
    # (63, 256) and (20, 32): max_bins > n, so numBins = n
    X, y = rows(n, d, n + max_bins)
    check(ctx, X, y, max_bins=max_bins)


def test_duplicates_and_constant_columns(ctx):
    X, y = rows(500, 6, 11)
    Q = np.round(X * 4) / 4          # quarter steps: duplicates, some columns distinct <= numSplits
    Q[:, 1] = np.round(X[:, 1])      # a handful of values
    check(ctx, Q, y)
    check(ctx, Q, y, max_bins=256)
    Q[:, 0] = 2.5                    # constant columns among the others
    Q[:, 5] = -0.0
    check(ctx, Q, y)
    K = np.full((100, 4), 3.25)      # every column constant: a single leaf
    t = check(ctx, K, (np.arange(100) % 3 == 0).astype(np.float64))
    assert len(t[0]) == 1
    for lab in (0.0, 1.0):           # one class: a pure root
        t = check(ctx, X, np.full(500, lab))
        assert len(t[0]) == 1 and t[0][0]["predict"] == lab


def test_extreme_values(ctx):
    rng = np.random.default_rng(3)
    X, y = rows(400, 5, 13)
    X[:, 0] = rng.choice([-0.0, 0.0, 1.0, -1.0], 400)
    X[:, 1] = rng.choice([0.0, 5e-324, -5e-324, 2e-310, -2e-310, 1e-300], 400)
    X[:, 2] = rng.choice([1e300, -1e300, 1.7e308, -1.7e308, 0.0], 400)
    y = ((X[:, 0] > 0) ^ (X[:, 1] > 0) ^ (X[:, 2] > 0)).astype(np.float64)
    check(ctx, X, y)
    check(ctx, X, y, max_bins=4)


@pytest.mark.parametrize("max_depth", [0, 1, 5])
def test_max_depth(ctx, max_depth):
    X, y = rows(600, 7, 17)
    t = check(ctx, X, y, max_depth=max_depth)
    assert len(t[0]) <= 2 ** (max_depth + 1) - 1 and (max_depth > 0 or len(t[0]) == 1)


def max_active(t, max_depth):
    """The most nodes of one level that get a histogram (not leaves when they are made)."""
    level = np.floor(np.log2(t["id"])).astype(int)
    return int(np.bincount(level[(t["impurity"] != 0.0) & (level < max_depth)]).max())


@pytest.mark.parametrize("d", [4, 48])
def test_deep_tree_runs_node_groups(ctx, d):
    # random labels, depth 12: hundreds of nodes.  One histogram launch holds 32768 / (d * 32 * 2)
    # nodes in LDS: 128 at d = 4, which no level of this tree exceeds, and 10 at d = 48, where the
    # deeper levels take up to ten groups
    rng = np.random.default_rng(19)
    X = rng.standard_normal((4096, d))
    y = rng.integers(0, 2, 4096).astype(np.float64)
    t = check(ctx, X, y, max_depth=12)
    assert len(t[0]) > 500
    if d == 48:
        assert max_active(t[0], 12) > 3 * (32768 // (d * 32 * 2))


def test_one_tree_level_larger_than_a_group(ctx):
    """1024 features at 256 bins: a node's aggregates are 256 * 2 * 1024 * 8 B = 4 MB, so a group
    of the node queue (maxMemoryInMB = 256) is 64 nodes, and a level of one tree with more active
    nodes than that leaves the queue in several groups: routing one group must leave the rows of
    the nodes still queued alone.  The restatement is too slow at 1024 features to run here, so
    the tree is held to its own rows instead: X routed down it in numpy.  The features are random
    bits, the labels random: every candidate halves its node, so the tree stays full.  (Off the
    device, the restatement on these rows has 89 active nodes at level 7, and 128 with 8 features;
    Gaussian features under random labels split a few rows off at a time and reach 19.)"""
    n, d, depth = 2048, 1024, 8
    rng = np.random.default_rng(29)
    X = rng.integers(0, 2, (n, d)).astype(np.float64)
    y = rng.integers(0, 2, n).astype(np.float64)
    t = clf.dtree_train(ctx, X, y, max_bins=256, max_depth=depth)
    # dtree::nodes_valid's conditions
    at, inner = np.arange(len(t)), t["feature"] >= 0
    assert np.all(t["feature"] >= -1) and np.all(t["feature"] < d)
    assert np.all(t["left"][~inner] == -1) and np.all(t["right"][~inner] == -1)
    for side in ("left", "right"):
        assert np.all(t[side][inner] > at[inner]) and np.all(t[side][inner] < len(t))
    assert np.array_equal(t["id"][t["left"][inner]], 2 * t["id"][inner])
    assert np.array_equal(t["id"][t["right"][inner]], 2 * t["id"][inner] + 1)
    # the class counts of every node, by routing the rows down the tree
    counts = np.zeros((len(t), 2), dtype=np.int64)
    where, live, lab = np.zeros(n, dtype=np.int64), np.arange(n), y.astype(np.int64)
    while live.size:
        np.add.at(counts, (where[live], lab[live]), 1)
        live = live[t["feature"][where[live]] >= 0]
        a = where[live]
        left = X[live, t["feature"][a]] <= t["threshold"][a]
        where[live] = np.where(left, t["left"][a], t["right"][a])
    total = counts.sum(axis=1)
    assert total[0] == n and np.all(total >= 1)
    assert np.array_equal(total[t["left"][inner]] + total[t["right"][inner]], total[inner])
    assert np.array_equal(t["predict"], (counts[:, 1] > counts[:, 0]).astype(np.float64))
    assert np.array_equal(t["impurity"], R.impurity("gini", counts[:, 0], counts[:, 1]))
    assert np.array_equal(clf.dtree_predict(ctx, X, t), t["predict"][where])
    # a level with more nodes that get a histogram than one group holds
    assert len(t) < 2 ** (depth + 1) and max_active(t, depth) > 64


@pytest.mark.parametrize("mi", [1, 5, 300])
def test_min_instances_per_node(ctx, mi):
    X, y = rows(300, 4, 23)
    t = check(ctx, X, y, min_instances_per_node=mi)
    assert mi < 300 or len(t[0]) == 1


@pytest.mark.parametrize("seed", [0, 12345])
def test_sampled_thresholds(ctx, seed):
    # n > max(max_bins^2, 10000): the thresholds come from Spark's Bernoulli sample of the rows
    n = 10050
    X, y = rows(n, 3, 29)
    kept = clf.spark_sample(n, 10000 / n, 1, seed)
    assert 0 < kept.size < n
    check(ctx, X, y, sample_rows=kept, split_seed=seed, max_bins=8, max_depth=3)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    got = clf.dtree_train(ctx, Xd, yd, max_bins=8, max_depth=3, split_seed=seed)
    same_tree(got, R.train(X, y, "gini", max_bins=8, max_depth=3, sample_rows=kept))
    # a non-finite value in a row outside the sample is the bin kernel's to find
    out = np.setdiff1d(np.arange(n), kept)[0]
    X[out, 1] = np.inf
    with pytest.raises(fx.EegfxError, match="not finite"):
        clf.dtree_train(ctx, X, y, max_bins=8, max_depth=3, split_seed=seed)


def test_device_inputs_and_reproducibility(ctx):
    X, y = rows(1000, 48, 31)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    P = probes(X, 7)
    for kind in KINDS:
        want = R.train(X, y, kind)
        a = clf.dtree_train(ctx, Xd, yd, impurity=kind)
        b = clf.dtree_train(ctx, Xd, yd, impurity=kind)
        h = clf.dtree_train(ctx, X, y, impurity=kind)
        same_tree(a, want)
        assert a.tobytes() == b.tobytes() == h.tobytes()
        for Z in (X, P, P[:0], P[:65]):
            p = clf.dtree_predict(ctx, torch.from_numpy(Z).cuda(), a)
            torch.cuda.synchronize()
            assert np.array_equal(p.cpu().numpy(), R.predict(want, Z))
    with pytest.raises(ValueError):
        clf.dtree_train(ctx, Xd, y)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_training_rows_are_refused(ctx, bad):
    X, y = rows(200, 5, 37)
    X[137, 3] = bad
    for A, b in ((X, y), (torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())):
        with pytest.raises(fx.EegfxError, match="not finite") as e:
            clf.dtree_train(ctx, A, b)
        assert e.value.code == _lib.EEGFX_EINVAL


def test_labels_other_than_0_and_1_are_refused(ctx):
    X, y = rows(200, 5, 41)
    y[77] = 0.5
    with pytest.raises(fx.EegfxError, match="validation") as e:
        clf.dtree_train(ctx, X, y)
    assert e.value.code == _lib.EEGFX_EINVAL


def test_argument_checks(ctx):
    X, y = rows(16, 2, 43)
    nodes = np.zeros(63, dtype=clf.TREE_NODE)
    count = c_int32()

    def train(n=16, d=2, imp=0, depth=5, bins=32, mi=1, cap=63, mem=0, Xp=X, np_=nodes):
        return fx.lib().eegfx_dtree_train(ctx.handle, _lib.ptr(Xp), _lib.ptr(y), n, d, imp, depth,
                                          bins, mi, 0, _lib.ptr(np_), cap, byref(count), mem)

    assert train() == _lib.EEGFX_OK and 1 <= count.value <= 31
    needed = count.value
    assert train(mem=2) == _lib.EEGFX_EINVAL
    assert train(n=1) == _lib.EEGFX_EINVAL
    assert train(n=0) == _lib.EEGFX_EINVAL
    assert train(d=0) == _lib.EEGFX_EINVAL
    assert train(d=1025) == _lib.EEGFX_EINVAL
    assert train(Xp=None) == _lib.EEGFX_EINVAL
    assert train(imp=2) == _lib.EEGFX_EINVAL
    assert train(bins=1) == _lib.EEGFX_EINVAL
    assert train(bins=257) == _lib.EEGFX_ENOTSUP
    assert train(depth=31) == _lib.EEGFX_EINVAL
    assert train(depth=-1) == _lib.EEGFX_EINVAL
    assert train(mi=0) == _lib.EEGFX_EINVAL
    # mem is checked before the sizes, the sizes before the parameters
    assert train(mem=2, n=1, bins=257) == _lib.EEGFX_EINVAL
    assert train(n=1, bins=257) == _lib.EEGFX_EINVAL
    if needed > 1:  # too small an array: the count needed comes back
        count.value = 0
        assert train(cap=needed - 1) == _lib.EEGFX_EINVAL and count.value == needed
    with pytest.raises(ValueError):
        clf.dtree_train(ctx, X, y, impurity="variance")


def test_predict_refuses_a_corrupt_model(ctx):
    X, y = rows(300, 4, 47)
    good = clf.dtree_train(ctx, X, y)
    assert len(good) >= 3
    out = np.zeros(300)

    def predict(nodes, n=300, d=4, n_nodes=None, mem=0):
        return fx.lib().eegfx_dtree_predict(ctx.handle, _lib.ptr(X), n, d, _lib.ptr(nodes),
                                            len(nodes) if n_nodes is None else n_nodes,
                                            _lib.ptr(out), mem)

    assert predict(good) == _lib.EEGFX_OK
    assert predict(good, mem=7) == _lib.EEGFX_EINVAL
    assert predict(good, n=-1) == _lib.EEGFX_EINVAL
    assert predict(good, n_nodes=0) == _lib.EEGFX_EINVAL
    assert predict(good, d=int(good["feature"].max())) == _lib.EEGFX_EINVAL  # a feature >= d
    for field, value in (("left", len(good)), ("right", 0), ("left", -1), ("right", 1 << 30),
                         ("feature", 4), ("feature", -7)):
        bad = good.copy()
        bad[0][field] = value
        assert predict(bad) == _lib.EEGFX_EINVAL, (field, value)
    bad = good.copy()  # truncated: children past the end
    assert predict(bad, n_nodes=len(good) - 1) == _lib.EEGFX_EINVAL
    with pytest.raises(fx.EegfxError):
        clf.dtree_predict(ctx, X, bad[:1])


def test_classifier_flow_on_info_txt(ctx, golden_vectors):
    """ClassifierTest's flow with train_clf=dt: provider -> shuffle / split -> train -> test."""
    from eeg_dataanalysispackage_amd.pipeline import reference_split, train_test_features
    odp = fx.OffLineDataProvider([INFO_TRAIN], context=ctx)
    odp.loadData()
    fe = fx.WaveletTransform(8, 512, 175, 16, context=ctx)
    Xtr, ytr, Xte, yte = train_test_features(odp, fe)
    data, labels = odp.getData(), odp.getDataLabels()
    tr, te = reference_split(len(labels))
    assert list(tr) == [0, 7, 9, 2, 5, 10, 6] and list(te) == [3, 1, 8, 4]
    c = fx.DecisionTreeClassifier(context=ctx)
    with pytest.raises(RuntimeError):
        c.test(data[te], [labels[i] for i in te])
    for config, kw in (({}, {}),
                       ({"config_max_bins": "4", "config_impurity": "entropy",
                         "config_max_depth": "2", "config_min_instances_per_node": "2"},
                        dict(impurity_kind="entropy", max_bins=4, max_depth=2,
                             min_instances_per_node=2)),
                       ({"config_max_bins": "8", "config_impurity": "Gini",  # not "gini": Entropy
                         "config_max_depth": "3", "config_min_instances_per_node": "1"},
                        dict(impurity_kind="entropy", max_bins=8, max_depth=3)),
                       ({"config_max_bins": "4", "config_impurity": "entropy"}, {})):  # incomplete
        c.setConfig(config)
        c.train(data[tr], [labels[i] for i in tr], fe)
        want = R.train(np.asarray(Xtr), np.asarray(ytr), **kw)
        same_tree(c.nodes, want)
        pred = R.predict(want, np.asarray(Xte))
        assert np.array_equal(c.predict(np.asarray(Xte)), pred)
        if len(set(np.asarray(yte).tolist())) == 2:
            stats = c.test(data[te], [labels[i] for i in te])
            assert stats.as_tuple() == clf.reference_statistics(pred, yte).as_tuple()
            assert stats.getNumberOfPatterns() == len(te)
    # one actual class in the test split: the reference's cm[1] throws, and so does this
    one = [i for i in range(len(labels)) if labels[i] == labels[te[0]]]
    with pytest.raises(IndexError):
        c.test(data[one], [labels[i] for i in one])
