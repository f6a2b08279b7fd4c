"""train_clf=rf on the GPU (csrc/rforest.hip, eegfx_rforest_*) against the Python restatement of
MLlib 1.6.2 RandomForest (tests/rforest_reference.py, pinned by tests/test_rforest_reference.py).
The bagging weights and the weighted histograms are integers and the gains the same IEEE
operations, so the bar is equality: every node of every tree, the offsets and the predictions,
under both impurities.  Parity with Spark itself is unpinned."""
from ctypes import byref, c_int32

import numpy as np
import pytest
import torch

import rforest_reference as R
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd import classification as clf
from conftest import INFO_TRAIN
from test_gpu_dtree import probes, rows, same_tree

pytestmark = pytest.mark.gpu
KINDS = ("gini", "entropy")


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0, numerics="exact")
    yield c
    c.close()


def same_forest(got, want):
    assert got[1].dtype == np.int32 and got[1].tolist() == want[1].tolist()
    same_tree(got[0], want[0])


def check(ctx, X, y, sample_rows=None, split_seed=0, num_trees=3, feature_subset="sqrt",
          num_partitions=2, seed=12345, **params):
    """Both impurities: the device's forest is the restatement's, and so are its predictions on
    the training rows, fresh rows, rows with NaN / Inf, and no rows at all.  Returns the device's
    forests and the restatement's (nodes, offsets, subsets, group sizes)."""
    P = probes(X, 5)
    W = R.bag(X.shape[0], num_trees, num_partitions, seed)   # the same bag under both impurities
    out = []
    for kind in KINDS:
        got = clf.rforest_train(ctx, X, y, impurity=kind, split_seed=split_seed,
                                num_trees=num_trees, feature_subset=feature_subset, seed=seed,
                                num_partitions=num_partitions, **params)
        want = R.train(X, y, kind, sample_rows=sample_rows, num_trees=num_trees,
                       feature_subset=feature_subset, seed=seed, num_partitions=num_partitions,
                       weights=W, **params)
        same_forest(got, want)
        for Z in (X, P, P[:0]):
            assert np.array_equal(clf.rforest_predict(ctx, Z, *got), R.predict(*want[:2], Z))
        out.append((got, want))
    return out


@pytest.mark.parametrize("d", [1, 3, 48, 65, 130])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 1000])
def test_forest_matches_restatement(ctx, n, d):
    X, y = rows(n, d, 1000 * n + d)
    (got, _), _ = check(ctx, X, y)
    if n >= 257:
        assert len(got[0]) > 9  # the shapes grow real trees


def test_the_reference_default(ctx):
    # RandomForestClassifier.java without a complete config: 100 trees, "auto" (sqrt: 7 of 48)
    X, y = rows(1000, 48, 53)
    (got, want), _ = check(ctx, X, y, num_trees=100, feature_subset="auto")
    assert len(got[1]) == 101 and all(len(f) == 7 for f in want[2].values())


@pytest.mark.parametrize("subset", R.SUBSETS)
def test_every_subset_name(ctx, subset):
    X, y = rows(257, 48, 59)
    k = {"auto": 7, "all": 48, "sqrt": 7, "log2": 6, "onethird": 16}[subset]
    for (nodes, off), (_, _, drawn, _) in check(ctx, X, y, feature_subset=subset):
        trees = [nodes[off[t]:off[t + 1]] for t in range(3)]
        for t, tree in enumerate(trees):
            for nd in tree[tree["feature"] >= 0]:
                feats = drawn[(t, int(nd["id"]))]
                assert len(feats) == k and int(nd["feature"]) in feats
        assert sum(a.tobytes() != b.tobytes() for a, b in zip(trees, trees[1:] + trees[:1])) >= 2


@pytest.mark.parametrize("n,d,max_bins", [(1000, 48, 32), (257, 130, 256)])
@pytest.mark.parametrize("subset", ["auto", "all"])
def test_one_tree_is_the_decision_tree(ctx, n, d, max_bins, subset):
    X, y = rows(n, d, n + d)
    for kind in KINDS:
        tree = clf.dtree_train(ctx, X, y, impurity=kind, max_bins=max_bins)
        nodes, off = clf.rforest_train(ctx, X, y, impurity=kind, max_bins=max_bins, num_trees=1,
                                       feature_subset=subset, num_partitions=3)
        assert len(tree) > 3 and off.tolist() == [0, len(tree)]
        assert nodes.tobytes() == tree.tobytes()
        Z = probes(X, 3)
        assert np.array_equal(clf.rforest_predict(ctx, Z, nodes, off),
                              clf.dtree_predict(ctx, Z, tree))


def test_several_launches_per_group_in_lds(ctx):
    # random labels, depth 10, 8 trees, 7 of 48 features: a node's histogram is 7 * 32 * 2 = 448
    # counters, so one launch holds 32768 // 448 = 73 nodes in LDS.  The restatement's largest
    # group (a whole level of all eight trees) has more than 4 * 73 nodes: at least five launches.
    rng = np.random.default_rng(19)
    X = rng.standard_normal((4096, 48))
    y = rng.integers(0, 2, 4096).astype(np.float64)
    for (nodes, _), (_, _, _, sizes) in check(ctx, X, y, num_trees=8, max_depth=10):
        assert len(nodes) > 2000
        assert max(sizes) > 4 * (32768 // (7 * 32 * 2))   # at least five launches in one group


def test_several_launches_per_group_in_global_memory(ctx):
    # every one of 130 features at 256 bins: a node's 66,560 counters do not fit LDS, the launch
    # adds to device memory, 16 MB // 266,240 B = 63 nodes at a time.  Depth 4 with 12 trees, not
    # the depth 10 with 8 trees of the LDS case: the restatement evaluates 130 * 255 candidates a
    # node in Python, about 13 ms a node under Entropy (one math.log per count), and depth 10 grows
    # thousands of nodes, minutes of restatement.  What the case is for is kept and asserted: a
    # group (level 3 of the 12 trees) with more than 63 nodes, so several launches.
    rng = np.random.default_rng(23)
    X = rng.standard_normal((4096, 130))
    y = rng.integers(0, 2, 4096).astype(np.float64)
    for _, (_, _, _, sizes) in check(ctx, X, y, num_trees=12, max_depth=4, max_bins=256,
                                     feature_subset="all"):
        assert max(sizes) > (16 << 20) // (130 * 256 * 2 * 4) == 63


def test_bagging_partitions(ctx):
    X, y = rows(500, 6, 61)
    forests = []
    for P in (1, 4, 16):
        (got, _), _ = check(ctx, X, y, num_partitions=P)
        forests.append(got[0].tobytes())
    assert len(set(forests)) == 3   # the slices' samplers differ
    W = R.bag(64, 40, 4, 12345)
    assert (W == 0).any() and (W >= 3).any()
    assert np.array_equal(clf.poisson_bag(64, 40, 4, 12345), W)
    X, y = rows(64, 5, 67)
    check(ctx, X, y, num_trees=40, num_partitions=4)
    (a, _), _ = check(ctx, X, y, seed=-99)   # another seed: another bag, other subsets
    assert a[0].tobytes() != check(ctx, X, y)[0][0][0].tobytes()


@pytest.mark.parametrize("max_depth", [0, 1])
def test_max_depth(ctx, max_depth):
    X, y = rows(600, 7, 17)
    (got, _), _ = check(ctx, X, y, max_depth=max_depth)
    sizes = np.diff(got[1])
    assert np.all(sizes <= 2 ** (max_depth + 1) - 1) and (max_depth > 0 or np.all(sizes == 1))


@pytest.mark.parametrize("mi", [1, 5, 300])
def test_min_instances_per_node(ctx, mi):
    # the bound is on the weighted counts: 300 is never met on both sides of a split
    X, y = rows(300, 4, 23)
    (got, _), _ = check(ctx, X, y, min_instances_per_node=mi)
    assert mi < 300 or len(got[0]) == 3


def test_sampled_thresholds(ctx):
    # n > max(max_bins^2, 10000): one threshold table from Spark's Bernoulli sample, for all trees
    n = 10050
    X, y = rows(n, 3, 29)
    kept = clf.spark_sample(n, 10000 / n, 1, 7)
    assert 0 < kept.size < n
    check(ctx, X, y, sample_rows=kept, split_seed=7, max_bins=8, max_depth=3)


def test_duplicates_constant_columns_and_one_class(ctx):
    X, y = rows(500, 6, 11)
    Q = np.round(X * 4) / 4          # quarter steps: duplicates, some columns distinct <= numSplits
    Q[:, 1] = np.round(X[:, 1])      # a handful of values
    check(ctx, Q, y, feature_subset="log2")
    check(ctx, Q, y, max_bins=256)
    Q[:, 0] = 2.5                    # constant columns among the others
    Q[:, 5] = -0.0
    check(ctx, Q, y)
    K = np.full((100, 4), 3.25)      # every column constant: every tree a single leaf
    (got, _), _ = check(ctx, K, (np.arange(100) % 3 == 0).astype(np.float64))
    assert got[1].tolist() == [0, 1, 2, 3]
    for lab in (0.0, 1.0):           # one class: pure roots
        (got, _), _ = check(ctx, X, np.full(500, lab))
        assert len(got[0]) == 3 and np.all(got[0]["predict"] == lab)


def test_device_inputs_and_reproducibility(ctx):
    X, y = rows(1000, 48, 31)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    P = probes(X, 7)
    kw = dict(num_trees=5, num_partitions=2)
    for kind in KINDS:
        want = R.train(X, y, kind, **kw)
        a = clf.rforest_train(ctx, Xd, yd, impurity=kind, **kw)
        b = clf.rforest_train(ctx, Xd, yd, impurity=kind, **kw)
        h = clf.rforest_train(ctx, X, y, impurity=kind, **kw)
        same_forest(a, want)
        assert a[0].tobytes() == b[0].tobytes() == h[0].tobytes()
        assert a[1].tolist() == b[1].tolist() == h[1].tolist()
        for Z in (X, P, P[:0], P[:65]):
            p = clf.rforest_predict(ctx, torch.from_numpy(Z).cuda(), *a)
            torch.cuda.synchronize()
            assert np.array_equal(p.cpu().numpy(), R.predict(*want[:2], Z))
    with pytest.raises(ValueError):
        clf.rforest_train(ctx, Xd, y)


def test_a_tie_between_two_trees_is_class_0(ctx):
    X, y = rows(400, 6, 71)
    nodes, off = clf.rforest_train(ctx, X, y, num_trees=2, feature_subset="sqrt", num_partitions=2)
    want = R.train(X, y, num_trees=2, feature_subset="sqrt", num_partitions=2)
    same_forest((nodes, off), want)
    Z = np.concatenate([X, probes(X, 9)])
    votes = R.votes(nodes, off, Z)
    assert (votes == 1).any() and (votes == 2).any() and (votes == 0).any()
    got = clf.rforest_predict(ctx, Z, nodes, off)
    assert np.all(got[votes == 1] == 0.0)   # one vote each: a tie
    assert np.array_equal(got, (votes == 2).astype(np.float64))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_training_rows_are_refused(ctx, bad):
    X, y = rows(200, 5, 37)
    X[137, 3] = bad
    for A, b in ((X, y), (torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())):
        with pytest.raises(fx.EegfxError, match="not finite") as e:
            clf.rforest_train(ctx, A, b, num_trees=3)
        assert e.value.code == _lib.EEGFX_EINVAL
    # a row outside the threshold sample is the bin kernel's to find
    n = 10050
    X, y = rows(n, 3, 29)
    kept = clf.spark_sample(n, 10000 / n, 1, 0)
    X[np.setdiff1d(np.arange(n), kept)[0], 1] = bad
    with pytest.raises(fx.EegfxError, match="not finite"):
        clf.rforest_train(ctx, X, y, num_trees=2, max_bins=8, max_depth=2)


def test_labels_other_than_0_and_1_are_refused(ctx):
    X, y = rows(200, 5, 41)
    y[77] = 0.5
    with pytest.raises(fx.EegfxError, match="validation") as e:
        clf.rforest_train(ctx, X, y, num_trees=3)
    assert e.value.code == _lib.EEGFX_EINVAL


def test_argument_checks(ctx):
    X, y = rows(16, 2, 43)
    nodes = np.zeros(3 * 63, dtype=clf.TREE_NODE)
    off = np.zeros(4, dtype=np.int32)
    count = c_int32()

    def train(n=16, d=2, imp=0, depth=5, bins=32, mi=1, trees=3, subset=0, parts=2, cap=189, mem=0,
              Xp=X, yp=y, np_=nodes, op=off, cp=count):
        return fx.lib().eegfx_rforest_train(
            ctx.handle, _lib.ptr(Xp), _lib.ptr(yp), n, d, imp, depth, bins, mi, trees, subset,
            12345, parts, 0, _lib.ptr(np_), cap, _lib.ptr(op), None if cp is None else byref(cp), mem)

    assert train() == _lib.EEGFX_OK and 3 <= count.value <= 93 and off[3] == count.value
    needed = count.value
    assert train(parts=0) == _lib.EEGFX_OK   # the processors available to the process
    assert train(mem=2) == _lib.EEGFX_EINVAL
    assert train(n=1) == _lib.EEGFX_EINVAL
    assert train(n=0) == _lib.EEGFX_EINVAL
    assert train(d=0) == _lib.EEGFX_EINVAL
    assert train(d=1025) == _lib.EEGFX_EINVAL
    assert train(cap=-1) == _lib.EEGFX_EINVAL
    assert train(Xp=None) == _lib.EEGFX_EINVAL
    assert train(yp=None) == _lib.EEGFX_EINVAL
    assert train(np_=None) == _lib.EEGFX_EINVAL
    assert train(op=None) == _lib.EEGFX_EINVAL
    assert train(cp=None) == _lib.EEGFX_EINVAL
    assert train(imp=2) == _lib.EEGFX_EINVAL
    assert train(bins=1) == _lib.EEGFX_EINVAL
    assert train(bins=257) == _lib.EEGFX_ENOTSUP
    assert train(depth=31) == _lib.EEGFX_EINVAL
    assert train(depth=-1) == _lib.EEGFX_EINVAL
    assert train(mi=0) == _lib.EEGFX_EINVAL
    assert train(trees=0) == _lib.EEGFX_EINVAL
    assert train(trees=-4) == _lib.EEGFX_EINVAL
    assert train(subset=5) == _lib.EEGFX_EINVAL
    assert train(subset=-1) == _lib.EEGFX_EINVAL
    assert train(parts=-1) == _lib.EEGFX_EINVAL
    # mem is checked before the sizes, the sizes before the parameters, the tree's before the
    # forest's
    assert train(mem=2, n=1, bins=257) == _lib.EEGFX_EINVAL
    assert train(n=1, bins=257) == _lib.EEGFX_EINVAL
    assert train(bins=257, trees=0) == _lib.EEGFX_ENOTSUP
    count.value = 0   # too small an array: the count needed comes back
    assert train(cap=needed - 1) == _lib.EEGFX_EINVAL and count.value == needed
    assert train(cap=0, np_=None) == _lib.EEGFX_EINVAL and count.value == needed
    with pytest.raises(ValueError):
        clf.rforest_train(ctx, X, y, impurity="variance")
    with pytest.raises(ValueError):
        clf.rforest_train(ctx, X, y, feature_subset="half")


def test_the_python_call_grows_its_node_array(ctx):
    # random labels, depth 14 on 6000 rows: more than the 1023 nodes a tree of the first guess
    rng = np.random.default_rng(73)
    X = rng.standard_normal((6000, 4))
    y = rng.integers(0, 2, 6000).astype(np.float64)
    nodes, off = clf.rforest_train(ctx, X, y, num_trees=1, max_depth=14)
    assert len(nodes) > 1023 and off.tolist() == [0, len(nodes)]
    assert nodes.tobytes() == clf.dtree_train(ctx, X, y, max_depth=14).tobytes()


def test_predict_refuses_a_corrupt_forest(ctx):
    X, y = rows(300, 4, 47)
    good, off = clf.rforest_train(ctx, X, y, num_trees=3, num_partitions=2)
    assert np.all(np.diff(off) >= 3)
    out = np.zeros(300)

    def predict(nodes, offsets=off, n=300, d=4, trees=3, mem=0, Xp=X, outp=out):
        offsets = np.ascontiguousarray(offsets, dtype=np.int32) if offsets is not None else None
        return fx.lib().eegfx_rforest_predict(ctx.handle, _lib.ptr(Xp), n, d, _lib.ptr(nodes),
                                              _lib.ptr(offsets), trees, _lib.ptr(outp), mem)

    assert predict(good) == _lib.EEGFX_OK
    assert np.array_equal(out, R.predict(good, off, X))
    assert predict(good, n=0, Xp=None, outp=None) == _lib.EEGFX_OK
    assert predict(good, mem=7) == _lib.EEGFX_EINVAL
    assert predict(good, n=-1) == _lib.EEGFX_EINVAL
    assert predict(good, d=0) == _lib.EEGFX_EINVAL
    assert predict(good, d=1025) == _lib.EEGFX_EINVAL
    assert predict(good, trees=0) == _lib.EEGFX_EINVAL
    assert predict(None) == _lib.EEGFX_EINVAL
    assert predict(good, offsets=None) == _lib.EEGFX_EINVAL
    assert predict(good, Xp=None) == _lib.EEGFX_EINVAL
    assert predict(good, outp=None) == _lib.EEGFX_EINVAL
    assert predict(good, d=int(good["feature"].max())) == _lib.EEGFX_EINVAL  # a feature >= d
    o = off.tolist()
    for bad_off in ([1] + o[1:], [o[0], o[2], o[1], o[3]], [o[0], o[1], o[1], o[3]],
                    [o[0], o[1] - 1, o[2], o[3]],     # tree 0 loses its last node: a child past it
                    [o[0], -1, o[2], o[3]]):
        assert predict(good, offsets=bad_off) == _lib.EEGFX_EINVAL, bad_off
    first = int(off[1])   # the root of tree 1
    for at, field, value in ((0, "left", int(off[1])),       # inside the array, past the tree
                             (first, "left", int(off[2] - off[1])), (first, "right", 0),
                             (first, "left", -1), (0, "right", 1 << 30), (first, "feature", 4),
                             (int(off[2]), "feature", -7)):
        bad = good.copy()
        bad[at][field] = value
        assert predict(bad) == _lib.EEGFX_EINVAL, (at, field, value)
    # truncated: the last tree's last node is gone from the array and from the offsets
    assert predict(good[:-1].copy(), offsets=o[:3] + [o[3] - 1]) == _lib.EEGFX_EINVAL
    with pytest.raises(ValueError):
        clf.rforest_predict(ctx, X, good[:-1], off)   # the array and the offsets disagree
    with pytest.raises(fx.EegfxError):
        clf.rforest_predict(ctx, X, good[:1], [0, 1])  # a root with children and nothing else


def test_classifier_flow_on_info_txt(ctx, golden_vectors):
    """ClassifierTest's flow with train_clf=rf: provider -> shuffle / split -> train -> test."""
    from eeg_dataanalysispackage_amd.pipeline import reference_split, train_test_features
    odp = fx.OffLineDataProvider([INFO_TRAIN], context=ctx)
    odp.loadData()
    fe = fx.WaveletTransform(8, 512, 175, 16, context=ctx)
    Xtr, ytr, Xte, yte = train_test_features(odp, fe)
    data, labels = odp.getData(), odp.getDataLabels()
    tr, te = reference_split(len(labels))
    c = fx.RandomForestClassifier(context=ctx)
    c.num_partitions = 2
    with pytest.raises(RuntimeError):
        c.test(data[te], [labels[i] for i in te])
    full = {"config_max_bins": "4", "config_impurity": "entropy", "config_max_depth": "2",
            "config_min_instances_per_node": "2", "config_feature_subset": "log2",
            "config_num_trees": "5"}
    for config, kw in (({}, {}),
                       (full, dict(impurity_kind="entropy", max_bins=4, max_depth=2,
                                   min_instances_per_node=2, feature_subset="log2", num_trees=5)),
                       (dict(full, config_impurity="Gini", config_feature_subset="onethird",
                             config_num_trees="1"),   # not "gini": Entropy
                        dict(impurity_kind="entropy", max_bins=4, max_depth=2,
                             min_instances_per_node=2, feature_subset="onethird", num_trees=1)),
                       ({k: v for k, v in full.items() if k != "config_num_trees"}, {})):
        c.setConfig(config)
        c.train(data[tr], [labels[i] for i in tr], fe)
        want = R.train(np.asarray(Xtr), np.asarray(ytr), num_partitions=2, **kw)
        same_forest((c.nodes, c.tree_offsets), want)
        assert len(c.tree_offsets) == kw.get("num_trees", 100) + 1
        pred = R.predict(*want[:2], np.asarray(Xte))
        assert np.array_equal(c.predict(np.asarray(Xte)), pred)
        if len(set(np.asarray(yte).tolist())) == 2:
            stats = c.test(data[te], [labels[i] for i in te])
            assert stats.as_tuple() == clf.reference_statistics(pred, yte).as_tuple()
            assert stats.getNumberOfPatterns() == len(te)
    c.setConfig(dict(full, config_feature_subset="half"))   # Spark's require
    with pytest.raises(ValueError, match="featureSubsetStrategy"):
        c.train(data[tr], [labels[i] for i in tr], fe)
