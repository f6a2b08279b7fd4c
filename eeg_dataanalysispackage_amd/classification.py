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
``NeuralNetworkClassifier`` (train_clf=nn) is the dense network the reference builds with DL4J from
its ``config_layer<i>_*`` keys, as DESIGN.md section 10.7 defines it (``eegfx_nn_train`` /
``eegfx_nn_predict`` / ``eegfx_nn_statistics``); its statistics follow
``ClassificationStatistics.add``, not Spark's confusion matrix.
``sgd_train_sharded`` / ``svm_sgd_train_sharded`` / ``count_sharded`` (and the classifiers'
``trainShards`` / ``testShards``) are the two SGD classifiers over rows that stay on the contexts of
a sharded provider (``eegfx_glm_sgd_train_sharded`` / ``eegfx_glm_count_sharded``, DESIGN.md section
10.11); one driver trains behind both sets of entries, a lone context being its one shard.
Model save/load (Spark model directories) is out of scope.
"""
from __future__ import annotations

import math
from ctypes import byref, c_int32, c_int64
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import EegfxError, lib, ptr
from .context import Context, _check_out, _contig, _is_device, _mem

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


def _start_weights(d, initial_weights):
    """The [d] array a train entry reads the initial weights from (None: zeros, as MLlib) and
    writes the result to: the caller's own array is never written."""
    w = (np.zeros(d) if initial_weights is None
         else np.array(initial_weights, dtype=np.float64).copy())
    if w.shape != (d,):
        raise ValueError(f"initial_weights must be [{d}]")
    return w


def _train(entry, ctx: Context, X, y, num_iterations, step_size, reg_param, mini_batch_fraction,
           convergence_tol, initial_weights, num_partitions=None):
    X, y, n, d, mem = _train_inputs(X, y)
    w = _start_weights(d, initial_weights)
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


# ---- the SGD classifiers over rows that stay on several contexts ------

def _glm_shards(shards, with_pos=True):
    """``shards``: (context, X, y[, pos]) per shard -- device tensors on the context's device, X
    [n][d] float64, y [n] float64, pos [n] int64 or None.  Returns the eegfx_glm_shard array, what
    keeps its tensors alive, d, and the (context, tensor) pairs to order the streams by."""
    import torch
    arr = (_lib.GlmShard * max(1, len(shards)))()
    keep, order, d = [], [], None
    for i, sh in enumerate(shards):
        ctx, X, y = sh[0], sh[1], sh[2]
        pos = sh[3] if len(sh) > 3 and with_pos else None
        if not (_is_device(X) and _is_device(y)) or (pos is not None and not _is_device(pos)):
            raise ValueError("the rows of a shard are device tensors")
        X, y = _contig(X, np.float64), _contig(y, np.float64)
        if X.ndim != 2 or y.ndim != 1 or int(y.shape[0]) != int(X.shape[0]):
            raise ValueError(f"X must be [n][d] and y [n], got {tuple(X.shape)} and "
                             f"{tuple(y.shape)}")
        if d is None:
            d = int(X.shape[1])
        if int(X.shape[1]) != d:
            raise ValueError(f"shard {i} has {int(X.shape[1])} features, shard 0 has {d}")
        n = int(X.shape[0])
        if pos is not None:
            pos = pos.contiguous()
            if pos.dtype != torch.int64 or tuple(pos.shape) != (n,):
                raise ValueError(f"pos must be int64 [{n}]")
        keep.append((X, y, pos))
        arr[i] = _lib.GlmShard(ctx.handle, ptr(X) if n else None, ptr(y) if n else None,
                               ptr(pos) if n and pos is not None else None, n)
        if n:
            order.append((ctx, X))
    return arr, keep, d, order


def _call_sharded(order, fn, *args):
    """Context._call over several contexts: every context's stream is ordered after the torch
    work that produced its shard's tensors, and torch's streams after the call."""
    pairs = [ctx._enter_device(ref) for ctx, ref in order]
    try:
        _lib.check(fn(*args))
    finally:
        for (ctx, _), pair in zip(order, pairs):
            ctx._leave_device(pair)


def _train_sharded(grad, shards, num_iterations, step_size, reg_param, mini_batch_fraction,
                   convergence_tol, initial_weights, num_partitions):
    arr, keep, d, order = _glm_shards(shards)
    if d is None:
        raise ValueError("no shards")
    w = _start_weights(d, initial_weights)
    it = c_int32()
    parts = 1 if num_partitions is None else int(num_partitions)
    _call_sharded(order, lib().eegfx_glm_sgd_train_sharded, grad, arr, len(shards), d,
                  int(num_iterations), float(step_size), float(reg_param),
                  float(mini_batch_fraction), float(convergence_tol), parts, ptr(w), byref(it))
    return w, it.value


def sgd_train_sharded(shards, num_iterations: int = DEFAULT_NUM_ITERATIONS,
                      step_size: float = DEFAULT_STEP_SIZE, reg_param: float = 0.0,
                      mini_batch_fraction: float = DEFAULT_MINI_BATCH_FRACTION,
                      convergence_tol: float = CONVERGENCE_TOL, initial_weights=None,
                      num_partitions: Optional[int] = None):
    """sgd_train over rows that stay where they are (eegfx_glm_sgd_train_sharded: the driver
    sgd_train runs with its context as the one shard).  ``shards``: (context, X, y[, pos]) per
    shard, each context once; pos names the position of every row in the whole training list
    (None: the shards' rows in shard order), the list mini_batch_fraction < 1 samples
    (num_partitions None: the processors available to the process).
    Returns (weights, iterations_run); one shard is sgd_train's run, bit for bit."""
    if num_partitions is None and mini_batch_fraction < 1.0:
        num_partitions = int(lib().eegfx_available_processors())
    return _train_sharded(0, shards, num_iterations, step_size, reg_param, mini_batch_fraction,
                          convergence_tol, initial_weights, num_partitions)


def svm_sgd_train_sharded(shards, num_iterations: int = DEFAULT_NUM_ITERATIONS,
                          step_size: float = DEFAULT_STEP_SIZE,
                          reg_param: float = DEFAULT_REG_PARAM,
                          mini_batch_fraction: float = DEFAULT_MINI_BATCH_FRACTION,
                          convergence_tol: float = CONVERGENCE_TOL, initial_weights=None):
    """svm_sgd_train (full batch) over rows that stay where they are; see sgd_train_sharded."""
    return _train_sharded(1, shards, num_iterations, step_size, reg_param, mini_batch_fraction,
                          convergence_tol, initial_weights, None)


def shard_state(ctx: Context, d: int):
    """(iterations, flag, updates, weights) of the training state the last SGD run left on ``ctx``
    (eegfx_glm_shard_state), whichever entry ran it: on every shard that took part, the root's
    bits; after sgd_train / svm_sgd_train, the returned weights'."""
    head = np.zeros(4, dtype=np.int32)
    w = np.empty(d, dtype=np.float64)
    _lib.check(lib().eegfx_glm_shard_state(ctx.handle, int(d), ptr(head), ptr(w)))
    return int(head[0]), int(head[1]), int(head[2]), w


def count_sharded(shards, weights, intercept: float = 0.0, threshold: Optional[float] = 0.5,
                  svm: bool = False):
    """(tp, tn, fp, fn) of the model's predictions over every shard's rows, scored and counted in
    one kernel where the rows are (eegfx_glm_count_sharded): what predict / svm_predict followed
    by confusion_counts gives on the rows together.  ``shards``: (context, X, y) per shard.
    Raises as confusion_counts does."""
    arr, keep, d, order = _glm_shards(shards, with_pos=False)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if d is None:
        d = int(w.shape[0])
    if w.shape != (d,):
        raise ValueError(f"weights must be [{d}]")
    counts = np.zeros(4, dtype=np.int64)
    t = math.nan if threshold is None else float(threshold)
    _call_sharded(order, lib().eegfx_glm_count_sharded, 1 if svm else 0, arr, len(shards), d,
                  ptr(w), float(intercept), t, ptr(counts))
    return tuple(int(v) for v in counts)


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
                 falseNegatives: int = 0, MSE: Optional[float] = None,
                 class1sum: Optional[float] = None, class2sum: Optional[float] = None):
        self.truePositives = int(truePositives)
        self.trueNegatives = int(trueNegatives)
        self.falsePositives = int(falsePositives)
        self.falseNegatives = int(falseNegatives)
        # what add() accumulates besides the counters (train_clf=nn); printed only when set
        self._has_sums = not (MSE is None and class1sum is None and class2sum is None)
        self.MSE = float(MSE or 0.0)
        self.class1sum = float(class1sum or 0.0)
        self.class2sum = float(class2sum or 0.0)

    def getNumberOfPatterns(self) -> int:
        return self.truePositives + self.trueNegatives + self.falsePositives + self.falseNegatives

    def calcAccuracy(self) -> float:
        n = self.getNumberOfPatterns()
        return (self.truePositives + self.trueNegatives) / n if n else math.nan

    def as_tuple(self):
        return (self.truePositives, self.trueNegatives, self.falsePositives, self.falseNegatives)

    def __repr__(self) -> str:
        text = (f"Number of patterns: {self.getNumberOfPatterns()}\n"
                f"True positives: {self.truePositives}\nTrue negatives: {self.trueNegatives}\n"
                f"False positives: {self.falsePositives}\n"
                f"False negatives: {self.falseNegatives}\n"
                f"Accuracy: {self.calcAccuracy() * 100}%\n")
        if self._has_sums:
            n = self.getNumberOfPatterns()
            text += (f"MSE: {self.MSE / n if n else math.nan}\n"
                     f"Non-targets: {self.class1sum}\nTargets: {self.class2sum}\n")
        return text


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


def _pair_inputs(values, labels, what):
    """A (values, labels) pair for a device count: both host or both device, contiguous float64,
    both [n].  Returns (values, labels, n, mem)."""
    if _is_device(values) != _is_device(labels):
        raise ValueError(f"{what} and labels must both be host or both be device arrays")
    v = _contig(values, np.float64)
    a = _contig(labels, np.float64)
    n = int(v.shape[0])
    if v.ndim != 1 or a.ndim != 1 or int(a.shape[0]) != n:
        raise ValueError(f"{what} and labels must be [n], got {tuple(v.shape)} and "
                         f"{tuple(a.shape)}")
    return v, a, n, _mem(v, a)


def confusion_counts(ctx: Context, predictions, labels):
    """(tp, tn, fp, fn) as reference_statistics reads them, counted on the device in one pass
    (eegfx_confusion_counts): only the four integers come back.  predictions and labels are both
    host arrays or both device tensors.  Raises IndexError where reference_statistics does (one
    actual class, or no rows) and EegfxError for a label that is neither 0.0 nor 1.0."""
    p, a, n, mem = _pair_inputs(predictions, labels, "predictions")
    counts = np.zeros(4, dtype=np.int64)
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

    # The two hooks of test / testFeatures: the reference's statistics of host predictions, and
    # the same statistics counted on the device.
    def _host_statistics(self, predictions, labels) -> ClassificationStatistics:
        return reference_statistics(predictions, labels)

    def _device_statistics(self, predictions, labels) -> ClassificationStatistics:
        return ClassificationStatistics(*confusion_counts(self.context, predictions, labels))

    def test(self, epochs, targets: Sequence[float]) -> ClassificationStatistics:
        """The statistics of the epochs' predictions (the network: NeuralNetworkClassifier.java
        :152-168 -- resultsStats.add(output, target) per epoch)."""
        if not self._trained():
            raise RuntimeError("The classifier has not been trained")
        return self._host_statistics(self.predict(self._features(epochs)), targets)

    def testFeatures(self, X, y) -> ClassificationStatistics:
        """test() on feature rows that exist already.  Predictions of device rows stay on the
        device and are counted there (confusion_counts: four integers come back; the network's
        scores: nn_statistics); host rows go through reference_statistics (the network's:
        reference_nn_statistics) as test() does."""
        pred = self.predict(X)
        if not _is_device(pred):
            return self._host_statistics(pred, y)
        if not _is_device(y):
            import torch
            y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64), device=pred.device)
        return self._device_statistics(pred, y)


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
        self.weights, self.iterations_run = sgd_train(self.context, X, y, **self._sgd_config())

    def _predict_rows(self, features):
        return predict(self.context, features, self.weights)

    # The flow over the provider's shards (OffLineDataProvider.splitShards): what trainFeatures /
    # testFeatures do on the rows together, with the rows left on their contexts.
    _SVM = False

    def _sgd_config(self):
        """trainFeatures' reading of the config as sgd_train's arguments."""
        c = self.config
        if all(k in c for k in ("config_num_iterations", "config_step_size",
                                "config_mini_batch_fraction")):
            return dict(num_iterations=int(c["config_num_iterations"]),
                        step_size=float(c["config_step_size"]), reg_param=0.0,
                        mini_batch_fraction=float(c["config_mini_batch_fraction"]),
                        num_partitions=self.num_partitions)
        return dict(num_iterations=DEFAULT_NUM_ITERATIONS, step_size=DEFAULT_STEP_SIZE,
                    reg_param=DEFAULT_REG_PARAM, mini_batch_fraction=DEFAULT_MINI_BATCH_FRACTION)

    def trainShards(self, split) -> None:
        """trainFeatures on the training part of OffLineDataProvider.splitShards(), each shard's
        rows on its own context (sgd_train_sharded)."""
        shards = [(s.context, s.X_train, s.y_train, s.pos_train) for s in split]
        fn = svm_sgd_train_sharded if self._SVM else sgd_train_sharded
        self.weights, self.iterations_run = fn(shards, **self._sgd_config())

    def testShards(self, split) -> ClassificationStatistics:
        """testFeatures on the test part of splitShards(): scored and counted where the rows
        are (count_sharded); the four integers of every shard come back."""
        if not self._trained():
            raise RuntimeError("The classifier has not been trained")
        shards = [(s.context, s.X_test, s.y_test) for s in split]
        return ClassificationStatistics(*count_sharded(
            shards, self.weights, threshold=0.0 if self._SVM else 0.5, svm=self._SVM))


class SVMClassifier(LogisticRegressionClassifier):
    """IClassifier for train_clf=svm (SVMClassifier.java), GPU-resident: the same flow and model
    attributes as LogisticRegressionClassifier with SVMWithSGD and SVMModel.predict."""

    def trainFeatures(self, X, y) -> None:
        """:83-111 -- with config_num_iterations / config_step_size / config_reg_param /
        config_mini_batch_fraction all set, the static SVMWithSGD.train(rdd, iterations, step,
        regParam, fraction); otherwise new SVMWithSGD().run (step 1.0, 100 iterations,
        regParam 0.01, fraction 1.0)."""
        self.weights, self.iterations_run = svm_sgd_train(self.context, X, y,
                                                          **self._sgd_config())

    def _predict_rows(self, features):
        return svm_predict(self.context, features, self.weights)

    _SVM = True

    def _sgd_config(self):
        c = self.config
        if all(k in c for k in ("config_num_iterations", "config_step_size", "config_reg_param",
                                "config_mini_batch_fraction")):
            return dict(num_iterations=int(c["config_num_iterations"]),
                        step_size=float(c["config_step_size"]),
                        reg_param=float(c["config_reg_param"]),
                        mini_batch_fraction=float(c["config_mini_batch_fraction"]))
        return dict(num_iterations=DEFAULT_NUM_ITERATIONS, step_size=DEFAULT_STEP_SIZE,
                    reg_param=DEFAULT_REG_PARAM, mini_batch_fraction=DEFAULT_MINI_BATCH_FRACTION)


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


# ---- train_clf=nn (NeuralNetworkClassifier.java) ------------------------
NN_LAYER_KEYS = ("layer_type", "drop_out", "activation_function", "n_out")
NN_GLOBAL_KEYS = ("config_seed", "config_num_iterations", "config_learning_rate",
                  "config_momentum", "config_weight_init", "config_updater",
                  "config_optimization_algo", "config_loss_function", "config_pretrain",
                  "config_backprop")
NN_WEIGHT_INITS = ("xavier", "zero", "sigmoid", "uniform", "relu")


@dataclass(frozen=True)
class NnModel:
    """A checked train_clf=nn model: d features, the layers' widths and activation names, the
    loss and updater names (unknown strings already mapped as the reference's parse* do), and the
    training settings.  optimization_algo other than stochastic_gradient_descent trains through
    eegfx_nn_train_opt with max_line_search_iterations trials a search."""
    d: int
    widths: Tuple[int, ...]
    activations: Tuple[str, ...]
    loss: str = "mse"
    updater: str = "nesterovs"
    learning_rate: float = 0.1
    momentum: float = 0.5
    num_iterations: int = 1000
    seed: int = 12345
    weight_init: str = "xavier"
    optimization_algo: str = "stochastic_gradient_descent"
    max_line_search_iterations: int = 5

    def optimizer(self) -> "_lib.NnOptimizer":
        o = _lib.NnOptimizer()
        o.algorithm = _lib.NN_OPTIMIZERS[self.optimization_algo]
        o.max_line_search_iterations = int(self.max_line_search_iterations)
        return o

    def struct(self, num_iterations: Optional[int] = None) -> "_lib.NnConfig":
        c = _lib.NnConfig()
        c.n_layers = len(self.widths)
        for i, (w, a) in enumerate(zip(self.widths[:_lib.NN_MAX_LAYERS], self.activations)):
            c.n_out[i] = int(w)
            c.activation[i] = _lib.NN_ACTIVATIONS[a]
        c.loss = _lib.NN_LOSSES[self.loss]
        c.updater = _lib.NN_UPDATERS[self.updater]
        c.num_iterations = int(self.num_iterations if num_iterations is None else num_iterations)
        c.learning_rate = float(self.learning_rate)
        c.momentum = float(self.momentum)
        return c

    def layer_shapes(self):
        """(n_in, n_out) of every layer."""
        n_in = (self.d,) + tuple(self.widths[:-1])
        return list(zip(n_in, self.widths))

    @property
    def param_count(self) -> int:
        """eegfx_nn_param_count (host only): raises EegfxError for a model the library refuses."""
        n = lib().eegfx_nn_param_count(int(self.d), byref(self.struct()))
        if n < 0:
            _lib.check(int(n))
        return int(n)


def _nn_refuse(code, key, value, why):
    raise EegfxError(code, f"{key}={value}: {why}")


NN_LINE_SEARCH_ALGOS = ("line_gradient_descent", "lbfgs", "conjugate_gradient")


def nn_config_from(config: Dict[str, str], d: int, line_search: bool = False) -> NnModel:
    """The model NeuralNetworkClassifier.java:102-137, 258-320 builds from the config_* keys, or
    EegfxError naming the key and the value for what this library does not train.  Layer i = 1..L
    reads config_layer<i>_{layer_type, drop_out, activation_function, n_out}; L = the number of
    config_layer* keys // 4.  Unknown strings map as the reference's parse* map them (activation ->
    sigmoid, loss -> mse, updater -> nesterovs, weight init -> relu, optimization algorithm ->
    stochastic_gradient_descent, layer type -> output).  Refused: a missing key (the reference
    dies on null), auto_encoder / rbm / graves_lstm layers, a dense last layer or an output layer
    that is not last, dropout, pretrain=true, backprop other than true, more than 4 layers, hidden
    widths outside [1, 64], an output width other than 2 -- and, unless line_search is true, the
    line-search optimisers (line_gradient_descent, conjugate_gradient, lbfgs): with it they become
    NnModel.optimization_algo (DL4J's five line-search trials) and nn_train runs them."""
    def get(key):
        if key not in config or config[key] is None:
            raise EegfxError(_lib.EEGFX_EINVAL, f"{key} is missing (the reference dies on null)")
        return str(config[key])

    def number(key, kind):
        try:
            return kind(get(key))
        except ValueError:
            _nn_refuse(_lib.EEGFX_EINVAL, key, get(key), f"not {kind.__name__}")

    for key in NN_GLOBAL_KEYS:
        get(key)
    n_layers = sum(1 for k in config if k.startswith("config_layer")) // 4
    if not 1 <= n_layers <= _lib.NN_MAX_LAYERS:
        raise EegfxError(_lib.EEGFX_EINVAL,
                         f"{n_layers} layers (the config_layer* keys // 4): 1 to "
                         f"{_lib.NN_MAX_LAYERS} are supported")
    algo = get("config_optimization_algo")
    if algo in NN_LINE_SEARCH_ALGOS and not line_search:
        _nn_refuse(_lib.EEGFX_ENOTSUP, "config_optimization_algo", algo,
                   "a line-search optimiser: pass line_search=True to train under it")
    if get("config_pretrain") == "true":
        _nn_refuse(_lib.EEGFX_ENOTSUP, "config_pretrain", "true", "no layer here pretrains")
    if get("config_backprop") != "true":
        _nn_refuse(_lib.EEGFX_ENOTSUP, "config_backprop", get("config_backprop"),
                   "without backprop nothing is trained")
    widths, acts = [], []
    for i in range(1, n_layers + 1):
        pre = f"config_layer{i}_"
        kind = get(pre + "layer_type")
        if kind in ("auto_encoder", "rbm", "graves_lstm"):
            _nn_refuse(_lib.EEGFX_ENOTSUP, pre + "layer_type", kind,
                       "only dense and output layers are trained")
        if kind == "dense" and i == n_layers:
            _nn_refuse(_lib.EEGFX_EINVAL, pre + "layer_type", kind,
                       "the last layer must be an output layer")
        if kind != "dense" and i < n_layers:
            _nn_refuse(_lib.EEGFX_EINVAL, pre + "layer_type", kind,
                       "an output layer must be the last layer")
        if kind in ("dense", "output"):  # the default branch of parseLayer reads no drop_out
            drop = number(pre + "drop_out", float)
            if drop != 0.0:
                _nn_refuse(_lib.EEGFX_ENOTSUP, pre + "drop_out", get(pre + "drop_out"),
                           "dropout is not trained")
        width = number(pre + "n_out", int)
        if i < n_layers and not 1 <= width <= _lib.NN_MAX_WIDTH:
            _nn_refuse(_lib.EEGFX_EINVAL, pre + "n_out", width,
                       f"a dense layer's width lies in [1, {_lib.NN_MAX_WIDTH}]")
        if i == n_layers and width != 2:
            _nn_refuse(_lib.EEGFX_EINVAL, pre + "n_out", width,
                       "the output layer's n_out must be 2 (the labels are {t, |1 - t|})")
        act = get(pre + "activation_function")
        widths.append(width)
        acts.append(act if act in _lib.NN_ACTIVATIONS else "sigmoid")
    loss = get("config_loss_function")
    updater = get("config_updater")
    init = get("config_weight_init")
    iterations = number("config_num_iterations", int)
    if iterations < 0:
        _nn_refuse(_lib.EEGFX_EINVAL, "config_num_iterations", iterations, "negative")
    return NnModel(d=int(d), widths=tuple(widths), activations=tuple(acts),
                   loss=loss if loss in _lib.NN_LOSSES else "mse",
                   updater=updater if updater in _lib.NN_UPDATERS else "nesterovs",
                   learning_rate=number("config_learning_rate", float),
                   momentum=number("config_momentum", float), num_iterations=iterations,
                   seed=number("config_seed", int),
                   weight_init=init if init in NN_WEIGHT_INITS else "relu",
                   optimization_algo=(algo if algo in NN_LINE_SEARCH_ALGOS
                                      else "stochastic_gradient_descent"))


def nn_init_params(model: NnModel) -> np.ndarray:
    """The initial flat parameter vector (layer after layer: W[n_in][n_out] row-major, then
    b[n_out] = 0), drawn on the host.  ND4J's stream cannot be restated, so the generator is this
    one: ``rng = numpy.random.Generator(numpy.random.PCG64(seed & 0xFFFFFFFF))``; for each layer
    in order its n_in * n_out weights come from one call, in row-major order --
    xavier: ``rng.standard_normal(k) * sqrt(2 / (n_in + n_out))``;
    relu: ``rng.standard_normal(k) * sqrt(2 / n_in)``;
    sigmoid: ``rng.uniform(-a, a, k)`` with a = 4 sqrt(6 / (n_in + n_out));
    uniform: ``rng.uniform(-a, a, k)`` with a = 1 / sqrt(n_in); zero: zeros (no draw)."""
    rng = np.random.Generator(np.random.PCG64(int(model.seed) & 0xFFFFFFFF))
    parts = []
    for n_in, n_out in model.layer_shapes():
        k = n_in * n_out
        if model.weight_init == "xavier":
            w = rng.standard_normal(k) * math.sqrt(2.0 / (n_in + n_out))
        elif model.weight_init == "sigmoid":
            a = 4.0 * math.sqrt(6.0 / (n_in + n_out))
            w = rng.uniform(-a, a, k)
        elif model.weight_init == "uniform":
            a = 1.0 / math.sqrt(n_in)
            w = rng.uniform(-a, a, k)
        elif model.weight_init == "zero":
            w = np.zeros(k)
        else:
            w = rng.standard_normal(k) * math.sqrt(2.0 / n_in)
        parts += [w, np.zeros(n_out)]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)


def nn_train(ctx: Context, X, y, model: NnModel, params0=None, num_iterations=None,
             params_out=None, scores_out=None):
    """model.num_iterations (or num_iterations) full-batch iterations on the device
    (eegfx_nn_train) from params0 (default nn_init_params(model)); returns (params, scores):
    the trained flat vector and the loss before each iteration's step.  X (n x d float64) and y
    (n labels 0/1) are both host arrays or both device tensors; the results are host arrays
    (params_out / scores_out: caller's float64 buffers to fill instead of new ones)."""
    if model.optimization_algo != "stochastic_gradient_descent":
        return nn_train_opt(ctx, X, y, model, params0, num_iterations, params_out, scores_out)[:2]
    X, y, n, d, mem, cfg, p0, out, scores = _nn_train_args(X, y, model, params0, num_iterations,
                                                           params_out, scores_out)
    ctx._call(mem, X, lib().eegfx_nn_train, ctx.handle, ptr(X), ptr(y), n, d, byref(cfg), ptr(p0),
              ptr(out), ptr(scores), mem)
    return out, scores


def _nn_train_args(X, y, model, params0, num_iterations, params_out, scores_out):
    X, y, n, d, mem = _train_inputs(X, y)
    if d != model.d:
        raise ValueError(f"X has {d} features, the model {model.d}")
    cfg = model.struct(num_iterations)
    count = model.param_count
    p0 = np.ascontiguousarray(nn_init_params(model) if params0 is None else params0,
                              dtype=np.float64)
    if p0.shape != (count,):
        raise ValueError(f"params0 must hold {count} parameters, got {p0.shape}")
    out = (np.empty(count, dtype=np.float64) if params_out is None
           else _check_out(params_out, (count,)))
    scores = (np.empty(max(cfg.num_iterations, 0), dtype=np.float64) if scores_out is None
              else _check_out(scores_out, (max(cfg.num_iterations, 0),)))
    return X, y, n, d, mem, cfg, p0, out, scores


NN_SEARCH_DTYPE = np.dtype([("step", np.float64), ("score", np.float64), ("trials", np.int32),
                            ("pad", np.int32)])


def nn_train_opt(ctx: Context, X, y, model: NnModel, params0=None, num_iterations=None,
                 params_out=None, scores_out=None, search_out=None):
    """nn_train under model.optimization_algo (eegfx_nn_train_opt):
    returns (params, scores, search, iterations_run).  scores[i] is the loss at the start of
    iteration i and search[i] (NN_SEARCH_DTYPE: step, score, trials) what its line search
    returned; arrays made here end at iterations_run, a caller's scores_out / search_out
    (num_iterations entries) keeps what it held from there on.  stochastic_gradient_descent is
    eegfx_nn_train itself: iterations_run = num_iterations and search stays as it was."""
    X, y, n, d, mem, cfg, p0, out, scores = _nn_train_args(X, y, model, params0, num_iterations,
                                                           params_out, scores_out)
    iters = max(cfg.num_iterations, 0)
    if search_out is None:
        search = np.zeros(iters, dtype=NN_SEARCH_DTYPE)
    else:
        search = search_out
        if (not isinstance(search, np.ndarray) or search.dtype != NN_SEARCH_DTYPE
                or search.shape != (iters,) or not search.flags.c_contiguous):
            raise ValueError(f"search_out must be a contiguous NN_SEARCH_DTYPE array of {iters}")
    opt = model.optimizer()
    run = c_int32(0)
    ctx._call(mem, X, lib().eegfx_nn_train_opt, ctx.handle, ptr(X), ptr(y), n, d, byref(cfg),
              byref(opt), ptr(p0), ptr(out), ptr(scores), ptr(search), byref(run), mem)
    done = int(run.value)
    return (out, scores[:done] if scores_out is None else scores,
            search[:done] if search_out is None else search, done)


def nn_predict(ctx: Context, X, model: NnModel, params, out=None):
    """Output 0 of the last layer for every row of X (eegfx_nn_predict): the score of "target"
    the reference reads with model.output(features).getDouble(0); on X's side."""
    p = np.ascontiguousarray(params, dtype=np.float64)
    X, fresh, mem, n, d = _predict_inputs(X)
    if out is None:
        out = fresh
    else:
        mem = _mem(X, _check_out(out, (n,)))
    if d != model.d or p.shape != (model.param_count,):
        raise ValueError("X or params do not fit the model")
    cfg = model.struct()
    ctx._call(mem, X, lib().eegfx_nn_predict, ctx.handle, ptr(X), n, d, byref(cfg), ptr(p),
              ptr(out), mem)
    return out


def java_round(x: float) -> int:
    """Java 7+ Math.round(double): floor(x + 1/2) without the rounding error of the addition,
    NaN -> 0, saturating at Long.MIN_VALUE / MAX_VALUE."""
    x = float(x)
    if x != x:
        return 0
    if x >= 2.0 ** 63:
        return 2 ** 63 - 1
    if x <= -2.0 ** 63:
        return -2 ** 63
    f = math.floor(x)
    return f + (1 if x - f >= 0.5 else 0)


def reference_nn_statistics(scores, labels) -> ClassificationStatistics:
    """Utils/ClassificationStatistics.add(score, label) over the pairs, in order (:68-83): a label
    that rounds to 0 is a true negative if the score rounds to 0, else a false positive; a label
    that rounds to 1 a true positive if the score rounds to 1, else a false negative (a score
    that rounds to 2 or -1 is a miss, not dropped); MSE, class1sum and class2sum accumulate."""
    tp = tn = fp = fn = 0
    mse = c1 = c2 = 0.0
    for s, a in zip(np.asarray(scores, dtype=np.float64).tolist(),
                    np.asarray(labels, dtype=np.float64).tolist()):
        mse += (a - s) * (a - s)
        want, got = java_round(a), java_round(s)
        if want == 0:
            tn, fp = tn + (got == 0), fp + (got != 0)
            c1 += s
        elif want == 1:
            tp, fn = tp + (got == 1), fn + (got != 1)
            c2 += s
    return ClassificationStatistics(tp, tn, fp, fn, MSE=mse, class1sum=c1, class2sum=c2)


def nn_statistics(ctx: Context, scores, labels) -> ClassificationStatistics:
    """reference_nn_statistics counted on the device in one pass (eegfx_nn_statistics): the four
    counters are exact, the three sums are added in the kernel's fixed order.  scores and labels
    are both host arrays or both device tensors."""
    s, a, n, mem = _pair_inputs(scores, labels, "scores")
    counts = np.zeros(4, dtype=np.int64)
    sums = np.zeros(3, dtype=np.float64)
    ctx._call(mem, s, lib().eegfx_nn_statistics, ctx.handle, ptr(s), ptr(a), n, ptr(counts),
              ptr(sums), mem)
    return ClassificationStatistics(*(int(v) for v in counts), MSE=float(sums[0]),
                                    class1sum=float(sums[1]), class2sum=float(sums[2]))


class NeuralNetworkClassifier(_Classifier):
    """IClassifier for train_clf=nn (NeuralNetworkClassifier.java), GPU-resident: the dense
    network of DESIGN.md section 10.7.  ``model`` (NnModel), ``params`` (the flat vector) and
    ``scores`` (the loss per iteration) are set by training."""

    def __init__(self, context: Optional[Context] = None):
        super().__init__(context)
        self.model: Optional[NnModel] = None
        self.params: Optional[np.ndarray] = None
        self.scores: Optional[np.ndarray] = None

    def _trained(self) -> bool:
        return self.params is not None

    def trainFeatures(self, X, y) -> None:
        """:69-149 -- the network of the config_* keys (nn_config_from: every key is required, as
        in the reference), initialised by nn_init_params from config_seed and config_weight_init,
        fitted by config_num_iterations full-batch iterations under config_optimization_algo."""
        self.model = nn_config_from(self.config, int(X.shape[1]), line_search=True)
        self.params, self.scores = nn_train(self.context, X, y, self.model)

    def _predict_rows(self, features):
        return nn_predict(self.context, features, self.model, self.params)

    def _host_statistics(self, scores, labels) -> ClassificationStatistics:
        return reference_nn_statistics(scores, labels)

    def _device_statistics(self, scores, labels) -> ClassificationStatistics:
        return nn_statistics(self.context, scores, labels)


__all__ = ["ClassificationStatistics", "DecisionTreeClassifier", "LogisticRegressionClassifier",
           "NeuralNetworkClassifier", "NnModel", "RandomForestClassifier", "SVMClassifier",
           "java_round", "nn_config_from", "nn_init_params", "nn_predict", "nn_statistics",
           "nn_train", "nn_train_opt", "reference_nn_statistics", "confusion_counts",
           "dtree_predict", "dtree_train", "poisson_bag", "predict", "reference_statistics", "rforest_predict",
           "rforest_train", "sgd_train", "spark_sample", "svm_predict", "svm_sgd_train", "EegfxError"]
