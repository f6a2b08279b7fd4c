"""The downstream classifiers of the train/test flow on the GPU.

Mirrors ``Classification/LogisticRegressionClassifier`` and ``Classification/SVMClassifier``
(IClassifier) and
``Utils/ClassificationStatistics`` of the reference: ``train(epochs, targets, fe)`` extracts the
features of the epochs (one batched device call instead of the Spark map of :90) and fits Spark
MLlib 1.6.2 ``LogisticRegressionWithSGD`` on the device (``eegfx_logreg_sgd_train``);
``test(epochs, targets)`` predicts on the device and builds the statistics exactly as :117-141 do,
including the reference's reading of the column-major confusion matrix (its "false positives"
count actual-1 / predicted-0).  ``SVMClassifier`` is the same flow with MLlib 1.6.2
``SVMWithSGD`` (HingeGradient, ``eegfx_svm_sgd_train``) and ``SVMModel.predict`` (margin > 0).
``DecisionTreeClassifier`` (train_clf=dt) is the flow again with MLlib 1.6.2 ``DecisionTree``
(``eegfx_dtree_train`` / ``eegfx_dtree_predict``), and
``RandomForestClassifier`` (train_clf=rf) with MLlib 1.6.2 ``RandomForest``
(``eegfx_rforest_train`` / ``eegfx_rforest_predict``).
Model save/load (Spark model directories) is out of scope.
"""
from __future__ import annotations

import math
from ctypes import byref, c_int32, c_int64
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import EegfxError, lib, ptr
from .context import Context, _contig, _is_device, _mem

# LogisticRegressionWithSGD() defaults (MLlib 1.6.2) and GradientDescent's convergence tolerance
DEFAULT_STEP_SIZE = 1.0
DEFAULT_NUM_ITERATIONS = 100
DEFAULT_REG_PARAM = 0.01
DEFAULT_MINI_BATCH_FRACTION = 1.0
CONVERGENCE_TOL = 0.001


def _train_inputs(X, y):
    """The (X, y) of every train call: contiguous float64 [n][d] and [n] on one side.  Returns
    them with n, d and the mem flag."""
    if _is_device(X) != _is_device(y):
        raise ValueError("X and y must both be host or both be device arrays")
    X = _contig(X, np.float64)
    y = _contig(y, np.float64)
    if X.ndim != 2 or y.ndim != 1 or int(y.shape[0]) != int(X.shape[0]):
        raise ValueError(f"X must be [n][d] and y [n], got {tuple(X.shape)} and {tuple(y.shape)}")
    return X, y, int(X.shape[0]), int(X.shape[1]), _mem(X, y)


def _predict_inputs(X):
    """The X of every predict call: contiguous float64 [n][d].  Returns it with the output (one
    float64 per row on X's side: a torch tensor on its device, else numpy), the mem flag, n, d."""
    X = _contig(X, np.float64)
    if X.ndim != 2:
        raise ValueError(f"X must be [n][d], got {tuple(X.shape)}")
    n, d = int(X.shape[0]), int(X.shape[1])
    if _is_device(X):
        import torch
        out = torch.empty(n, dtype=torch.float64, device=X.device)
    else:
        out = np.empty(n, dtype=np.float64)
    return X, out, _mem(X, out), n, d


def _train(entry, ctx: Context, X, y, num_iterations, step_size, reg_param, mini_batch_fraction,
           convergence_tol, initial_weights, num_partitions=None):
    X, y, n, d, mem = _train_inputs(X, y)
    w = (np.zeros(d) if initial_weights is None
         else np.array(initial_weights, dtype=np.float64).copy())
    it = c_int32()
    # ordered after the torch work that produced X / y (Context._call), like every device call
    head = (ctx.handle, ptr(X), ptr(y), n, d, int(num_iterations), float(step_size),
            float(reg_param), float(mini_batch_fraction), float(convergence_tol))
    if num_partitions is None:
        ctx._call(mem, X, getattr(lib(), entry), *head, ptr(w), byref(it), mem)
    else:
        ctx._call(mem, X, getattr(lib(), entry + "_partitioned"), *head, int(num_partitions),
                  ptr(w), byref(it), mem)
    return w, it.value


def _predict(entry, ctx: Context, X, weights, intercept, threshold):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    X, out, mem, n, d = _predict_inputs(X)
    t = math.nan if threshold is None else float(threshold)
    ctx._call(mem, X, getattr(lib(), entry), ctx.handle, ptr(X), n, d, ptr(w), float(intercept),
              t, ptr(out), mem)
    return out


def sgd_train(ctx: Context, X, y, num_iterations: int = DEFAULT_NUM_ITERATIONS,
              step_size: float = DEFAULT_STEP_SIZE, reg_param: float = 0.0,
              mini_batch_fraction: float = DEFAULT_MINI_BATCH_FRACTION,
              convergence_tol: float = CONVERGENCE_TOL, initial_weights=None,
              num_partitions: Optional[int] = None):
    """LogisticRegressionWithSGD on the device; returns (weights, iterations_run).  X (n x d
    float64, host numpy or device torch) and y (n labels 0/1) may live on either side.
    mini_batch_fraction < 1 samples iteration i's mini-batch as MLlib's data.sample(false, f,
    42 + i) over num_partitions Spark partitions (None: the processors available to the process,
    affinity and cgroup quota honoured, as Spark local[*]'s Runtime.availableProcessors();
    eegfx_logreg_sgd_train_partitioned)."""
    return _train("eegfx_logreg_sgd_train", ctx, X, y, num_iterations, step_size, reg_param,
                  mini_batch_fraction, convergence_tol, initial_weights, num_partitions)


def spark_sample(n: int, fraction: float, num_partitions: int, seed: int) -> np.ndarray:
    """RDD.sample(false, fraction, seed) of n rows in num_partitions slices (eegfx_spark_sample,
    host only): the kept row indices, ascending."""
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    kept = c_int64()
    from ._lib import check
    check(lib().eegfx_spark_sample(int(n), float(fraction), int(num_partitions), int(seed),
                                   ptr(words), byref(kept)))
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    rows = np.nonzero(bits)[0]
    assert rows.size == kept.value
    return rows


def predict(ctx: Context, X, weights, intercept: float = 0.0,
            threshold: Optional[float] = 0.5):
    """LogisticRegressionModel.predict on the device: 0/1 per row, or the score when
    ``threshold`` is None (clearThreshold)."""
    return _predict("eegfx_logreg_predict", ctx, X, weights, intercept, threshold)


def svm_sgd_train(ctx: Context, X, y, num_iterations: int = DEFAULT_NUM_ITERATIONS,
                  step_size: float = DEFAULT_STEP_SIZE, reg_param: float = DEFAULT_REG_PARAM,
                  mini_batch_fraction: float = DEFAULT_MINI_BATCH_FRACTION,
                  convergence_tol: float = CONVERGENCE_TOL, initial_weights=None):
    """Full-batch SVMWithSGD (HingeGradient) on the device; returns (weights, iterations_run)."""
    return _train("eegfx_svm_sgd_train", ctx, X, y, num_iterations, step_size, reg_param,
                  mini_batch_fraction, convergence_tol, initial_weights)


def svm_predict(ctx: Context, X, weights, intercept: float = 0.0,
                threshold: Optional[float] = 0.0):
    """SVMModel.predict on the device: margin w.x + b > threshold (0.0) -> 1 else 0, or the
    margin when ``threshold`` is None (clearThreshold)."""
    return _predict("eegfx_svm_predict", ctx, X, weights, intercept, threshold)


# Strategy.defaultStrategy("Classification") (MLlib 1.6.2)
DEFAULT_IMPURITY = "gini"
DEFAULT_MAX_DEPTH = 5
DEFAULT_MAX_BINS = 32
DEFAULT_MIN_INSTANCES_PER_NODE = 1
TREE_NODE = np.dtype(_lib.TreeNode)


def _impurity(impurity):
    kinds = {"gini": _lib.GINI, "entropy": _lib.ENTROPY}
    if impurity not in kinds:
        raise ValueError(f"impurity must be one of {sorted(kinds)}, got {impurity!r}")
    return kinds[impurity]


def dtree_train(ctx: Context, X, y, impurity: str = DEFAULT_IMPURITY,
                max_depth: int = DEFAULT_MAX_DEPTH, max_bins: int = DEFAULT_MAX_BINS,
                min_instances_per_node: int = DEFAULT_MIN_INSTANCES_PER_NODE,
                split_seed: int = 0) -> np.ndarray:
    """MLlib 1.6.2 DecisionTree (two classes, continuous features) on the device
    (eegfx_dtree_train); returns the nodes, ascending by Spark's node index, as a structured
    array (id, feature, left, right, threshold, predict, impurity, gain; a leaf has feature -1).
    X (n x d float64, host numpy or device torch) and y (n labels 0/1) may live on either side.
    impurity: "gini" or "entropy".  split_seed seeds the Bernoulli sample of the rows the
    thresholds come from when n > max(max_bins^2, 10000) (Spark draws it fresh on every run)."""
    kind = _impurity(impurity)
    X, y, n, d, mem = _train_inputs(X, y)
    # every leaf holds a row and no node lies below max_depth
    depth = min(max(int(max_depth), 0), 30)
    capacity = max(1, min(2 ** (depth + 1) - 1, 2 * n - 1))
    nodes = np.zeros(capacity, dtype=TREE_NODE)
    count = c_int32()
    ctx._call(mem, X, lib().eegfx_dtree_train, ctx.handle, ptr(X), ptr(y), n, d, kind,
              int(max_depth), int(max_bins), int(min_instances_per_node), int(split_seed),
              ptr(nodes), capacity, byref(count), mem)
    return nodes[:count.value].copy()


def dtree_predict(ctx: Context, X, nodes):
    """DecisionTreeModel.predict on the device (eegfx_dtree_predict): the 0/1 of the leaf each row
    of X (host numpy or device torch) reaches; left iff x[feature] <= threshold."""
    nodes = np.ascontiguousarray(nodes, dtype=TREE_NODE)
    X, out, mem, n, d = _predict_inputs(X)
    ctx._call(mem, X, lib().eegfx_dtree_predict, ctx.handle, ptr(X), n, d, ptr(nodes),
              int(nodes.shape[0]), ptr(out), mem)
    return out


# RandomForestClassifier.java:101-136 without a complete config
DEFAULT_NUM_TREES = 100
DEFAULT_FEATURE_SUBSET = "auto"
DEFAULT_FOREST_SEED = 12345
FEATURE_SUBSETS = {"auto": _lib.SUBSET_AUTO, "all": _lib.SUBSET_ALL, "sqrt": _lib.SUBSET_SQRT,
                   "log2": _lib.SUBSET_LOG2, "onethird": _lib.SUBSET_ONETHIRD}


def rforest_train(ctx: Context, X, y, impurity: str = DEFAULT_IMPURITY,
                  max_depth: int = DEFAULT_MAX_DEPTH, max_bins: int = DEFAULT_MAX_BINS,
                  min_instances_per_node: int = DEFAULT_MIN_INSTANCES_PER_NODE,
                  num_trees: int = DEFAULT_NUM_TREES, feature_subset: str = DEFAULT_FEATURE_SUBSET,
                  seed: int = DEFAULT_FOREST_SEED, num_partitions: Optional[int] = None,
                  split_seed: int = 0):
    """MLlib 1.6.2 RandomForest (two classes, continuous features) on the device
    (eegfx_rforest_train); returns (nodes, tree_offsets): the trees' nodes one tree after another,
    as dtree_train returns one tree (children relative to the tree's first node), and tree t's
    range tree_offsets[t]:tree_offsets[t + 1].  feature_subset: "auto", "all", "sqrt", "log2" or
    "onethird".  seed seeds the bagging weights and the feature subsets (the reference: 12345),
    num_partitions the slices of the training RDD the bagging samplers belong to (None: the
    processors available to the process, as for sgd_train); the other arguments are dtree_train's.
    num_trees = 1 with "auto" or "all" is dtree_train's tree."""
    kind = _impurity(impurity)
    X, y, n, d, mem = _train_inputs(X, y)
    if feature_subset not in FEATURE_SUBSETS:
        raise ValueError(f"feature_subset must be one of {sorted(FEATURE_SUBSETS)}, "
                         f"got {feature_subset!r}")
    trees = max(int(num_trees), 1)
    depth = min(max(int(max_depth), 0), 30)
    # a first guess; the call reports the count needed when the forest is larger
    capacity = max(1, trees * min(2 ** (depth + 1) - 1, 2 * n - 1, 1023))
    offsets = np.zeros(trees + 1, dtype=np.int32)
    count = c_int32()
    while True:
        nodes = np.zeros(capacity, dtype=TREE_NODE)
        count.value = 0
        try:
            ctx._call(mem, X, lib().eegfx_rforest_train, ctx.handle, ptr(X), ptr(y), n, d,
                      kind, int(max_depth), int(max_bins), int(min_instances_per_node),
                      int(num_trees), FEATURE_SUBSETS[feature_subset], int(seed),
                      0 if num_partitions is None else int(num_partitions), int(split_seed),
                      ptr(nodes), capacity, ptr(offsets), byref(count), mem)
        except EegfxError:
            if count.value <= capacity:
                raise
            capacity = count.value
            continue
        return nodes[:count.value].copy(), offsets


def rforest_predict(ctx: Context, X, nodes, tree_offsets):
    """RandomForestModel.predict on the device (eegfx_rforest_predict): 1.0 where more trees vote 1
    than 0 for the row of X (host numpy or device torch), 0.0 otherwise (a tie included)."""
    nodes = np.ascontiguousarray(nodes, dtype=TREE_NODE)
    offsets = np.ascontiguousarray(tree_offsets, dtype=np.int32)
    if offsets.ndim != 1 or offsets.shape[0] < 2 or int(offsets[-1]) != int(nodes.shape[0]):
        raise ValueError("tree_offsets must hold one offset per tree and end at len(nodes)")
    X, out, mem, n, d = _predict_inputs(X)
    ctx._call(mem, X, lib().eegfx_rforest_predict, ctx.handle, ptr(X), n, d, ptr(nodes),
              ptr(offsets), int(offsets.shape[0]) - 1, ptr(out), mem)
    return out


def poisson_bag(n: int, num_trees: int, num_partitions: int, seed: int) -> np.ndarray:
    """The bagging weights of rforest_train (eegfx_poisson_bag, host only): uint8
    [num_trees][n], Poisson(1) draws of one sampler per slice of the rows."""
    from ._lib import check
    w = np.zeros((max(int(num_trees), 0), max(int(n), 0)), dtype=np.uint8)
    check(lib().eegfx_poisson_bag(int(n), int(num_trees), int(num_partitions), int(seed), ptr(w)))
    return w


class ClassificationStatistics:
    """Utils/ClassificationStatistics.java (the counters the classifiers report)."""

    def __init__(self, truePositives: int = 0, trueNegatives: int = 0, falsePositives: int = 0,
                 falseNegatives: int = 0):
        self.truePositives = int(truePositives)
        self.trueNegatives = int(trueNegatives)
        self.falsePositives = int(falsePositives)
        self.falseNegatives = int(falseNegatives)

    def getNumberOfPatterns(self) -> int:
        return self.truePositives + self.trueNegatives + self.falsePositives + self.falseNegatives

    def calcAccuracy(self) -> float:
        n = self.getNumberOfPatterns()
        return (self.truePositives + self.trueNegatives) / n if n else math.nan

    def as_tuple(self):
        return (self.truePositives, self.trueNegatives, self.falsePositives, self.falseNegatives)

    def __repr__(self) -> str:
        return (f"Number of patterns: {self.getNumberOfPatterns()}\n"
                f"True positives: {self.truePositives}\nTrue negatives: {self.trueNegatives}\n"
                f"False positives: {self.falsePositives}\n"
                f"False negatives: {self.falseNegatives}\n"
                f"Accuracy: {self.calcAccuracy() * 100}%\n")


def reference_statistics(predictions, labels) -> ClassificationStatistics:
    """LogisticRegressionClassifier.test :129-137: MulticlassMetrics' confusion matrix (rows =
    actual, columns = predicted, labels ascending) flattened column-major by toArray and read as
    tn, fp, fn, tp = cm[0], cm[1], cm[2], cm[3].  Spark 1.6's ``labels`` are the classes of the
    ACTUAL labels only (``tpByClass.keys``, built from ``labelCountByClass``), and a prediction
    of a class outside them falls out of the matrix.  With a single actual class the matrix is 1x1
    and the reference's cm[1] throws; so does this (IndexError)."""
    p = np.asarray(predictions, dtype=np.float64)
    a = np.asarray(labels, dtype=np.float64)
    classes = sorted(set(a.tolist()))
    k = len(classes)
    cm = np.zeros((k, k), dtype=np.int64)
    idx = {c: i for i, c in enumerate(classes)}
    for ai, pi in zip(a.tolist(), p.tolist()):
        if pi in idx:
            cm[idx[ai], idx[pi]] += 1
    flat = cm.flatten(order="F")
    tn, fp, fn, tp = (int(flat[0]), int(flat[1]), int(flat[2]), int(flat[3]))
    return ClassificationStatistics(tp, tn, fp, fn)


def confusion_counts(ctx: Context, predictions, labels):
    """(tp, tn, fp, fn) as reference_statistics reads them, counted on the device in one pass
    (eegfx_confusion_counts): only the four integers come back.  predictions and labels are both
    host arrays or both device tensors.  Raises IndexError where reference_statistics does (one
    actual class, or no rows) and EegfxError for a label that is neither 0.0 nor 1.0."""
    if _is_device(predictions) != _is_device(labels):
        raise ValueError("predictions and labels must both be host or both be device arrays")
    p = _contig(predictions, np.float64)
    a = _contig(labels, np.float64)
    n = int(p.shape[0])
    if p.ndim != 1 or a.ndim != 1 or int(a.shape[0]) != n:
        raise ValueError(f"predictions and labels must be [n], got {tuple(p.shape)} and "
                         f"{tuple(a.shape)}")
    counts = np.zeros(4, dtype=np.int64)
    mem = _mem(p, a)
    ctx._call(mem, p, lib().eegfx_confusion_counts, ctx.handle, ptr(p), ptr(a), n, ptr(counts),
              mem)
    return tuple(int(v) for v in counts)


class _Classifier:
    """What the four IClassifiers share: the context, the feature extraction, the config, and the
    train / test flow around a subclass's trainFeatures, _trained and _predict_rows."""

    def __init__(self, context: Optional[Context] = None):
        self._ctx = context
        self.fe = None
        self.config: Dict[str, str] = {}
        # Spark partitions of the training RDD (mini-batch sampling, bagging); None = local[*]
        self.num_partitions: Optional[int] = None

    @property
    def context(self) -> Context:
        if self._ctx is None:
            self._ctx = Context(0)
        return self._ctx

    def setFeatureExtraction(self, fe) -> None:
        self.fe = fe

    def getFeatureExtraction(self):
        return self.fe

    def setConfig(self, config: Dict[str, str]) -> None:
        self.config = dict(config)

    def _features(self, epochs):
        if self.fe is None:
            raise ValueError("no feature extraction set")
        ep = np.ascontiguousarray(np.asarray(epochs, dtype=np.float64))
        return self.fe.extractFeaturesBatch(ep)

    def train(self, epochs, targets: Sequence[float], fe) -> None:
        """IClassifier.train: the features of the epochs (one batched device call), then
        trainFeatures, whose docstring names the reference lines and the config switches."""
        self.fe = fe
        self.trainFeatures(self._features(epochs), np.asarray(targets, dtype=np.float64))

    def predict(self, features) -> np.ndarray:
        if not self._trained():
            raise RuntimeError("The classifier has not been trained")  # IllegalStateException
        return self._predict_rows(features)

    def test(self, epochs, targets: Sequence[float]) -> ClassificationStatistics:
        if not self._trained():
            raise RuntimeError("The classifier has not been trained")
        return reference_statistics(self.predict(self._features(epochs)), targets)

    def testFeatures(self, X, y) -> ClassificationStatistics:
        """test() on feature rows that exist already.  Predictions of device rows stay on the
        device and are counted there (confusion_counts: four integers come back); host rows go
        through reference_statistics as test() does."""
        pred = self.predict(X)
        if not _is_device(pred):
            return reference_statistics(pred, y)
        if not _is_device(y):
            import torch
            y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64), device=pred.device)
        return ClassificationStatistics(*confusion_counts(self.context, pred, y))


class LogisticRegressionClassifier(_Classifier):
    """IClassifier for train_clf=logreg (LogisticRegressionClassifier.java), GPU-resident."""

    def __init__(self, context: Optional[Context] = None):
        super().__init__(context)
        self.weights: Optional[np.ndarray] = None
        self.iterations_run = 0

    def _trained(self) -> bool:
        return self.weights is not None

    def trainFeatures(self, X, y) -> None:
        """train() on feature rows that exist already (host arrays or device tensors, as
        OffLineDataProvider.split returns them).  :85-114 -- the config_* keys select the static
        train(...) (regParam 0.0), otherwise the default LogisticRegressionWithSGD().run
        (regParam 0.01)."""
        c = self.config
        if all(k in c for k in ("config_num_iterations", "config_step_size",
                                "config_mini_batch_fraction")):
            self.weights, self.iterations_run = sgd_train(
                self.context, X, y, num_iterations=int(c["config_num_iterations"]),
                step_size=float(c["config_step_size"]), reg_param=0.0,
                mini_batch_fraction=float(c["config_mini_batch_fraction"]),
                num_partitions=self.num_partitions)
        else:
            self.weights, self.iterations_run = sgd_train(
                self.context, X, y, DEFAULT_NUM_ITERATIONS, DEFAULT_STEP_SIZE, DEFAULT_REG_PARAM,
                DEFAULT_MINI_BATCH_FRACTION)

    def _predict_rows(self, features):
        return predict(self.context, features, self.weights)


class SVMClassifier(LogisticRegressionClassifier):
    """IClassifier for train_clf=svm (SVMClassifier.java), GPU-resident: the same flow and model
    attributes as LogisticRegressionClassifier with SVMWithSGD and SVMModel.predict."""

    def trainFeatures(self, X, y) -> None:
        """:83-111 -- with config_num_iterations / config_step_size / config_reg_param /
        config_mini_batch_fraction all set, the static SVMWithSGD.train(rdd, iterations, step,
        regParam, fraction); otherwise new SVMWithSGD().run (step 1.0, 100 iterations,
        regParam 0.01, fraction 1.0)."""
        c = self.config
        if all(k in c for k in ("config_num_iterations", "config_step_size", "config_reg_param",
                                "config_mini_batch_fraction")):
            self.weights, self.iterations_run = svm_sgd_train(
                self.context, X, y, num_iterations=int(c["config_num_iterations"]),
                step_size=float(c["config_step_size"]), reg_param=float(c["config_reg_param"]),
                mini_batch_fraction=float(c["config_mini_batch_fraction"]))
        else:
            self.weights, self.iterations_run = svm_sgd_train(
                self.context, X, y, DEFAULT_NUM_ITERATIONS, DEFAULT_STEP_SIZE, DEFAULT_REG_PARAM,
                DEFAULT_MINI_BATCH_FRACTION)

    def _predict_rows(self, features):
        return svm_predict(self.context, features, self.weights)


def _tree_config(c: Dict[str, str]) -> dict:
    """The four config_* keys both tree classifiers read, as arguments of dtree_train and
    rforest_train ("gini" is Gini, any other string Entropy)."""
    return dict(impurity="gini" if c["config_impurity"] == "gini" else "entropy",
                max_depth=int(c["config_max_depth"]), max_bins=int(c["config_max_bins"]),
                min_instances_per_node=int(c["config_min_instances_per_node"]))


class DecisionTreeClassifier(_Classifier):
    """IClassifier for train_clf=dt (DecisionTreeClassifier.java), GPU-resident: the flow of
    LogisticRegressionClassifier with MLlib's DecisionTree and DecisionTreeModel.predict."""

    CONFIG_KEYS = ("config_max_bins", "config_impurity", "config_max_depth",
                   "config_min_instances_per_node")

    def __init__(self, context: Optional[Context] = None):
        super().__init__(context)
        self.nodes: Optional[np.ndarray] = None
        # seed of the threshold sample of more than max(max_bins^2, 10000) rows
        self.split_seed = 0

    def _trained(self) -> bool:
        return self.nodes is not None

    def trainFeatures(self, X, y) -> None:
        """:85-127 -- Strategy.defaultStrategy("Classification") (Gini, depth 5, 32 bins, 1
        instance per node); with config_max_bins / config_impurity / config_max_depth /
        config_min_instances_per_node all set, those instead ("gini" is Gini, any other string
        Entropy)."""
        c = self.config
        kw = _tree_config(c) if all(k in c for k in self.CONFIG_KEYS) else {}
        self.nodes = dtree_train(self.context, X, y, split_seed=self.split_seed, **kw)

    def _predict_rows(self, features):
        return dtree_predict(self.context, features, self.nodes)


class RandomForestClassifier(DecisionTreeClassifier):
    """IClassifier for train_clf=rf (RandomForestClassifier.java), GPU-resident: the flow of
    DecisionTreeClassifier with MLlib's RandomForest and RandomForestModel.predict."""

    CONFIG_KEYS = DecisionTreeClassifier.CONFIG_KEYS + ("config_feature_subset",
                                                        "config_num_trees")

    def __init__(self, context: Optional[Context] = None):
        super().__init__(context)
        self.tree_offsets: Optional[np.ndarray] = None

    def trainFeatures(self, X, y) -> None:
        """:101-136 -- Strategy.defaultStrategy("Classification"), 100 trees, "auto", seed 12345;
        with all six config keys set, their values instead ("gini" is Gini, any other string
        Entropy; a feature subset that is no strategy's name is Spark's failed require)."""
        c = self.config
        kw = {}
        if all(k in c for k in self.CONFIG_KEYS):
            if c["config_feature_subset"] not in FEATURE_SUBSETS:
                raise ValueError("requirement failed: RandomForest given invalid "
                                 f"featureSubsetStrategy: {c['config_feature_subset']}")
            kw = dict(_tree_config(c), num_trees=int(c["config_num_trees"]),
                      feature_subset=c["config_feature_subset"])
        self.nodes, self.tree_offsets = rforest_train(
            self.context, X, y, num_partitions=self.num_partitions, split_seed=self.split_seed,
            **kw)

    def _predict_rows(self, features):
        return rforest_predict(self.context, features, self.nodes, self.tree_offsets)


__all__ = ["ClassificationStatistics", "DecisionTreeClassifier", "LogisticRegressionClassifier",
           "RandomForestClassifier", "SVMClassifier", "confusion_counts", "dtree_predict",
           "dtree_train", "poisson_bag", "predict", "reference_statistics", "rforest_predict",
           "rforest_train", "sgd_train", "spark_sample", "svm_predict", "svm_sgd_train", "EegfxError"]
