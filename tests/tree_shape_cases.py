"""The shapes at which the tree kernels (csrc/dtree.hip, csrc/rforest.hip, csrc/hist_lds.h) take a
path the other tree tests leave unrun: later trips of the capped grid-stride loops (A), the exact
boundaries of the histogram dispatch (B), and inputs whose one winning candidate sits in a chosen
lane, bin end or feature-list position (C).  DESIGN.md section 10.3 has the arithmetic.  Not a test
module: tests/test_tree_shape_cases.py asserts, on the restatements alone, the condition every case
exists for, and tests/test_gpu_tree_shapes.py holds the device to the restatements at these shapes.
Inputs, bags and restated models are built once a process and must be left unchanged.
"""
from collections import namedtuple

import numpy as np

import dtree_reference as D
import rforest_reference as R
from oracle.mllib_logreg import JavaRandom

KINDS = ("gini", "entropy")
FOREST_SEED = 12345         # RandomForestClassifier.java's seed: the bags and the feature subsets
LDS_COUNTERS = 32768        # kDtLdsCounters: uint32 counters of one workgroup's LDS histogram
HIST_ROWS_PER_TRIP = 256 * 16 * 8    # dt_hist<true,true>, rf_hist: grid cap x waves x rows a wave
ROUTE_ROWS_PER_TRIP = 2048 * 256     # rf_route's grid.x cap x threads
TREES_PER_TRIP = 1024                # rf_route's and rf_init's grid.y cap
PREDICT_ROWS_PER_TRIP = 8192 * 256   # dt_predict, rf_predict
GATHER_PER_TRIP = 4096 * 256         # dt_gather, elements

# trees = 0: dtree_train; otherwise rforest_train with `trees` trees, `subset`, `parts` partitions.
# data: "linear" rows(), "sixteenths" the same with X rounded to 1/16, "random" labels by coin,
# "decisive" y = X[:, f] > threshold s of f, "pair" the same with f the feature that the roots'
# draw puts at (tree, list position) = divmod(pair, k).  device: X and y as device tensors.
Case = namedtuple("Case",
                  "name n d max_bins max_depth seed data trees subset parts f s pair device",
                  defaults=("linear", 0, "all", 2, None, None, None, False))


def rows(n, d, seed):
    """test_gpu_dtree.rows (that module needs torch and a device to import)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = (X @ rng.standard_normal(d) + 0.5 * rng.standard_normal(n) > 0).astype(np.float64)
    return X, y


def probes(X, seed):
    """test_gpu_dtree.probes."""
    rng = np.random.default_rng(seed)
    d = X.shape[1]
    fresh = rng.standard_normal((77, d)) * 1.5
    odd = rng.standard_normal((9, d))
    for i, v in enumerate((np.nan, np.inf, -np.inf) * 3):
        odd[i, rng.integers(0, d)] = v
    odd[8, :] = np.nan
    return np.concatenate([fresh, odd])


# ---- A: later trips ------------------------------------------------------------------------------
A1 = Case("A1", 530000, 3, 32, 3, 101)
A2 = A1._replace(name="A2", trees=1, subset="sqrt")
A3 = [Case("A3-d3-sqrt", 40000, 3, 32, 2, 103, trees=3, subset="sqrt"),
      Case("A3-d65-all", 40000, 65, 32, 2, 103, trees=3),
      Case("A3-d130-bins256", 40000, 130, 256, 2, 103, "sixteenths", trees=3)]
A5 = Case("A5", 64, 5, 32, 2, 105, trees=1030, subset="sqrt")
A6 = Case("A6", 10050, 130, 8, 2, 106, device=True)
# A4: predict.  A depth-5 tree and a 3-tree forest of PREDICT_TRAIN, walked by PREDICT_N rows
PREDICT_N, PREDICT_D, PREDICT_SEED = 2200000, 2, 104
PREDICT_TRAIN = [Case("A4-tree", 2000, PREDICT_D, 32, 5, 104),
                 Case("A4-forest", 2000, PREDICT_D, 32, 5, 104, trees=3)]

# ---- B: exact boundaries -------------------------------------------------------------------------
B1_SHAPES = [(64, 32), (63, 32), (64, 256), (128, 128), (128, 129)]
B1 = [Case(f"B1-{'rf' if t else 'dt'}-d{d}-bins{b}", 1000, d, b, 2, 200 + d + b, trees=t)
      for d, b in B1_SHAPES for t in (0, 3)]
B2 = Case("B2", 8192, 4, 32, 12, 1, "random")
B2_LEVELS = {9: 99, 10: 138, 11: 170}   # active nodes a level, Gini (pinned by the CPU test)
# (d, trees, the pair that decides): k = 8 and 5 features a node, so 64 and 65 pairs: the last lane
# of a single trip, and a second trip for lane 0 alone.  (A second trip that is partly filled runs
# in test_gpu_rforest.py already: 700 pairs at the reference's default.)
B3 = [Case(f"B3-d{d}-trees{t}", 257, d, 32, 1, 300 + t, "pair", trees=t, subset="sqrt", pair=p)
      for d, t, p in ((64, 8, 63), (25, 13, 64))]

# ---- C: decisive lanes, bins and list positions ----------------------------------------------------
C_SPLITS = (0, 1, 15, 30)
C1_FEATURES = {64: (0, 1, 31, 32, 62, 63), 130: (0, 63, 64, 65, 127, 128, 129)}
C2_FEATURES = {64: (0, 63), 130: (64, 129)}


def c1(d, f, s):
    return Case(f"C1-d{d}-f{f}-s{s}", 512, d, 32, 1, 400 + d, "decisive", f=f, s=s)


def c2(d, f):
    return Case(f"C2-d{d}-f{f}", 512, d, 32, 1, 400 + d, "decisive", trees=3, f=f, s=15)


C3 = Case("C3", 512, 48, 32, 1, 448, "decisive", trees=100, subset="sqrt", f=47, s=15)
C3_POSITIONS = [0, 0, 0, 0, 1, 2, 2, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]


# ---- builders --------------------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def features_per_node(c):
    return R.features_per_node(c.subset, c.trees, c.d) if c.trees else c.d


def root_lists(c):
    """The feature lists the roots draw when they all leave the queue in one group: one draw a
    tree, ascending, from the forest's seed."""
    rng = JavaRandom(FOREST_SEED)
    k = features_per_node(c)
    return [R.reservoir(c.d, k, rng.next_long()) for _ in range(c.trees)]


def decisive_feature(c):
    if c.data == "pair":
        t, j = divmod(c.pair, features_per_node(c))
        return root_lists(c)[t][j]
    return c.f


def _inputs(c):
    if c.data == "random":
        rng = np.random.default_rng(c.seed)
        X = rng.standard_normal((c.n, c.d))
        return X, rng.integers(0, 2, c.n).astype(np.float64)
    X, y = _once(("rows", c.n, c.d, c.seed), lambda: rows(c.n, c.d, c.seed))
    if c.data == "sixteenths":
        X = np.round(X * 16) / 16
    if c.data in ("decisive", "pair"):
        f = decisive_feature(c)
        s = 15 if c.s is None else c.s
        y = (X[:, f] > D.thresholds(X[:, f], c.max_bins - 1)[s]).astype(np.float64)
    return X, y


def inputs(c):
    """(X, y) of a case; cases that differ in the call alone (A1 and A2) share their rows."""
    return _once(("inputs", c.n, c.d, c.seed, c.data, decisive_feature(c), c.s),
                 lambda: _inputs(c))


def split_seed(c):
    return c.seed


def sample_rows(c):
    """The rows the thresholds come from: Spark's Bernoulli sample where n is above
    required_samples(max_bins) (the library's host-only restatement of it, pinned by
    tests/test_spark_sample.py), None (every row) otherwise."""
    required = D.required_samples(c.max_bins)
    if c.n <= required:
        return None
    from eeg_dataanalysispackage_amd import classification as clf
    return _once(("sample", c.n, required, split_seed(c)),
                 lambda: clf.spark_sample(c.n, required / c.n, 1, split_seed(c)))


def bag(c):
    """The bag, drawn once per (n, trees, partitions) under the forest's seed."""
    return _once(("bag", c.n, c.trees, c.parts), lambda: R.bag(c.n, c.trees, c.parts, FOREST_SEED))


def train_args(c):
    """The keyword arguments clf.dtree_train / clf.rforest_train take besides the impurity."""
    kw = dict(max_depth=c.max_depth, max_bins=c.max_bins, split_seed=split_seed(c))
    if c.trees:
        kw.update(num_trees=c.trees, feature_subset=c.subset, num_partitions=c.parts,
                  seed=FOREST_SEED)
    return kw


def restated(c, kind):
    """D.train's nodes, or R.train's (nodes, offsets, drawn, group sizes)."""
    def make():
        X, y = inputs(c)
        kw = dict(max_depth=c.max_depth, max_bins=c.max_bins, sample_rows=sample_rows(c))
        if not c.trees:
            return D.train(X, y, kind, **kw)
        return R.train(X, y, kind, num_trees=c.trees, feature_subset=c.subset, seed=FOREST_SEED,
                       num_partitions=c.parts, weights=bag(c), **kw)
    return _once(("model", c, kind), make)


def predict_rows():
    """A4's rows to walk: Gaussian, as the training rows."""
    return _once(("predict rows",), lambda: np.random.default_rng(PREDICT_SEED + 1)
                 .standard_normal((PREDICT_N, PREDICT_D)))


def restated_predictions(c, kind):
    def make():
        m = restated(c, kind)
        Z = predict_rows()
        return R.predict(m[0], m[1], Z) if c.trees else D.predict(m, Z)
    return _once(("predictions", c, kind), make)


def active_per_level(tree, max_depth):
    """How many nodes of each level get a histogram (not leaves when they are made)."""
    level = np.floor(np.log2(tree["id"])).astype(int)
    return np.bincount(level[(tree["impurity"] != 0.0) & (level < max_depth)])


def tree_of(forest, t):
    nodes, off = forest[0], forest[1]
    return nodes[off[t]:off[t + 1]]
