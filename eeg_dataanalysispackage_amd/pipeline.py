"""Classifier-flow glue around the hot path.

Reproduces what ``PipelineBuilder.execute`` does between ``OffLineDataProvider`` and
``IClassifier.train/test`` (Pipeline/PipelineBuilder.java:167-188) so that GPU features feed the
same train/test split the reference uses:

* ``Collections.shuffle(data, new Random(1))`` and ``Collections.shuffle(targets, new Random(1))``
  (:177-179) -- the same permutation for both lists, from java.util.Random's 48-bit LCG;
* ``subList(0, (int)(size*0.7))`` / ``subList((int)(size*0.7), size)`` (:182-187);
* ``featureExtractionFunc`` + ``zip`` into ``LabeledPoint(label, features)``
  (Classification/LogisticRegressionClassifier.java:55-68, :87-94), batched on the device.

``run_train_clf`` is the whole ``train_clf`` branch (:170-223) with the rows resident on the device
from the provider to the four counters (``OffLineDataProvider.split``, ``trainFeatures``,
``testFeatures``); ``native_shuffle`` and ``gather_rows`` are its pieces over the C ABI.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

_MULT = 0x5DEECE66D
_MASK = (1 << 48) - 1


class JavaRandom:
    """java.util.Random (the 48-bit linear congruential generator of the JDK)."""

    def __init__(self, seed: int):
        self._seed = (seed ^ _MULT) & _MASK

    def _next(self, bits: int) -> int:
        self._seed = (self._seed * _MULT + 0xB) & _MASK
        v = self._seed >> (48 - bits)
        return v - (1 << bits) if v >= 1 << (bits - 1) and bits == 32 else v

    def nextInt(self, bound: int) -> int:
        if bound <= 0:
            raise ValueError("bound must be positive")
        if bound & (bound - 1) == 0:  # power of two
            return (bound * self._next(31)) >> 31
        while True:
            bits = self._next(31)
            val = bits % bound
            if bits - val + (bound - 1) < (1 << 31):  # no int overflow in Java
                return val


def java_shuffle_permutation(n: int, seed: int = 1) -> List[int]:
    """Index order after ``Collections.shuffle(list, new Random(seed))`` of a list of n items:
    ``for i = n..2: swap(list, i-1, rnd.nextInt(i))``."""
    idx = list(range(n))
    rnd = JavaRandom(seed)
    for i in range(n, 1, -1):
        j = rnd.nextInt(i)
        idx[i - 1], idx[j] = idx[j], idx[i - 1]
    return idx


def reference_split(n: int, seed: int = 1, train_fraction: float = 0.7
                    ) -> Tuple[List[int], List[int]]:
    """(train indices, test indices) into the provider's epoch list, as PipelineBuilder.java
    :177-187 slices the shuffled lists."""
    perm = java_shuffle_permutation(n, seed)
    cut = int(n * train_fraction)  # (int)(data.size()*0.7): truncation of a double
    return perm[:cut], perm[cut:]


def labeled_points(features, labels: Sequence[float]) -> List[Tuple[float, np.ndarray]]:
    """``new LabeledPoint(label, Vectors.dense(features))`` pairs (LogisticRegressionClassifier
    .java:63-68), in list order."""
    f = np.asarray(features)
    if len(f) != len(labels):
        raise ValueError("features and labels differ in length")
    return [(float(labels[i]), f[i]) for i in range(len(labels))]


def train_test_features(odp, fe) -> Tuple[np.ndarray, List[float], np.ndarray, List[float]]:
    """The reference's train/test data for a loaded provider: epochs shuffled and split like
    PipelineBuilder, features extracted in one batched device call per split (the Spark map of
    LogisticRegressionClassifier.java:90,126).  ``fe`` is a WaveletTransform."""
    data = odp.getData()
    labels = odp.getDataLabels()
    tr, te = reference_split(len(labels))
    ftr = fe.extractFeaturesBatch(np.ascontiguousarray(data[tr])) if tr else np.empty((0, 48))
    fte = fe.extractFeaturesBatch(np.ascontiguousarray(data[te])) if te else np.empty((0, 48))
    return ftr, [labels[i] for i in tr], fte, [labels[i] for i in te]


def native_shuffle(n: int, seed: int = 1) -> np.ndarray:
    """java_shuffle_permutation(n, seed) by the library (eegfx_java_shuffle, host only), as
    int64[n]."""
    from ._lib import check, lib, ptr
    perm = np.empty(max(int(n), 0), dtype=np.int64)
    check(lib().eegfx_java_shuffle(int(n), int(seed), ptr(perm)))
    return perm


def gather_rows(ctx, src, idx, out=None):
    """out[i] = src[idx[i]] on the device (eegfx_gather_rows), bits copied.  src: float64 [n][d]
    with 1 <= d <= 1536, or [n] (d = 1); idx: int64 [m], may repeat; all host arrays or all device
    tensors.  An index outside [0, n) raises IndexError and leaves that row of out alone."""
    from ._lib import lib, ptr
    from .context import _check_out, _contig, _empty_like_mem, _mem
    src = _contig(src, np.float64)
    idx = _contig(idx, np.int64)
    if src.ndim not in (1, 2) or idx.ndim != 1:
        raise ValueError(f"src must be [n][d] or [n] and idx [m], got {tuple(src.shape)} and "
                         f"{tuple(idx.shape)}")
    n, m = int(src.shape[0]), int(idx.shape[0])
    d = int(src.shape[1]) if src.ndim == 2 else 1
    shape = (m, d) if src.ndim == 2 else (m,)
    if out is None:
        out = _empty_like_mem(src, shape, "float64")
    _check_out(out, shape)
    mem = _mem(src, idx, out)
    ctx._call(mem, src, lib().eegfx_gather_rows, ctx.handle, ptr(src), n, d, ptr(idx), m,
              ptr(out), mem)
    return out


def run_train_clf(odp, classifier, fe=None, sharded=False):
    """PipelineBuilder.execute's train_clf branch (:170-223) for a loaded provider and one of the
    classifiers of :mod:`classification` (its config set by the caller): shuffle with Random(1),
    split 70/30, train, test; returns the ClassificationStatistics.  Epochs and feature rows stay
    on the device: what reaches the host is the model (and the tree's threshold sample) and the
    four counters.  ``fe``: a WaveletTransform, default (8, 512, 175, 16).  A classifier without
    a context of its own runs on the provider's first one.

    ``sharded=True`` (train_clf=logreg and train_clf=svm): the rows of a provider over several
    contexts stay on their shards (``splitShards``, ``trainShards``, ``testShards``): every shard
    sums the gradient of its own rows, d doubles per shard and iteration move, and the counters
    of the shards are added.  The other classifiers raise NotImplementedError."""
    from .feature_extraction import WaveletTransform
    if fe is None:
        fe = WaveletTransform(8, 512, 175, 16)
    if sharded:
        if not hasattr(classifier, "trainShards"):
            raise NotImplementedError(f"{type(classifier).__name__} has no sharded training: "
                                      "sharded=True serves train_clf=logreg and train_clf=svm")
        classifier.setFeatureExtraction(fe)
        split = odp.splitShards(fe)
        classifier.trainShards(split)
        return classifier.testShards(split)
    ctx = classifier._ctx
    if ctx is None and odp._ctxs:
        ctx = odp._ctxs[0]
    x_train, y_train, x_test, y_test = odp.split(fe, device=True, context=ctx)
    if classifier._ctx is None:
        classifier._ctx = ctx
    classifier.setFeatureExtraction(fe)
    classifier.trainFeatures(x_train, y_train)
    return classifier.testFeatures(x_test, y_test)
