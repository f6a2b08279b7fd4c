"""MLlib 1.6.2 DecisionTree as Classification/DecisionTreeClassifier.java:99-127 runs it (two
classes, continuous features), restated in Python floats from DESIGN.md section 10.  Not a test
module: tests/test_dtree_reference.py pins it by hand-worked cases and tests/test_gpu_dtree.py
compares the device with it, exactly.  It shares no code with the product.

Sums and products are numpy float64 element operations (IEEE, unfused, in the written order);
Entropy's logarithm is ``math.log``, one call per value, the libm the library links too.
"""
import math

import numpy as np

NODE = np.dtype([("id", "<i4"), ("feature", "<i4"), ("left", "<i4"), ("right", "<i4"),
                 ("threshold", "<f8"), ("predict", "<f8"), ("impurity", "<f8"), ("gain", "<f8")],
                align=True)
INVALID = -np.finfo(np.float64).max  # Double.MinValue: an invalid candidate's gain


def required_samples(max_bins):
    return max(max_bins * max_bins, 10000)


def thresholds(values, num_splits):
    """findSplitsForContinuousFeature over the sampled values of one feature."""
    val, cnt = np.unique(np.asarray(values, dtype=np.float64), return_counts=True)
    if len(val) <= num_splits:
        return [float(v) for v in val]
    out = []
    stride = len(values) / float(num_splits + 1)
    target = stride
    cur = int(cnt[0])
    for i in range(1, len(val)):
        prev = cur
        cur += int(cnt[i])
        if abs(prev - target) < abs(cur - target):
            out.append(float(val[i - 1]))
            target += stride
    return out


def _log2(f):
    flat = np.asarray(f, dtype=np.float64).ravel()
    ln2 = math.log(2.0)
    return np.array([math.log(v) / ln2 if v > 0.0 else 0.0 for v in flat.tolist()],
                    dtype=np.float64).reshape(np.shape(f))


def impurity(kind, c0, c1):
    """Gini: 1 - f0^2 - f1^2; Entropy: -f0 log2 f0 - f1 log2 f1 over the non-empty classes; 0 for
    an empty node.  c0 / c1: float64 arrays (or scalars) of class counts."""
    c0 = np.asarray(c0, dtype=np.float64)
    c1 = np.asarray(c1, dtype=np.float64)
    t = c0 + c1
    with np.errstate(invalid="ignore", divide="ignore"):
        f0, f1 = c0 / t, c1 / t
        if kind == "gini":
            imp = 1.0 - f0 * f0
            imp = imp - f1 * f1
        else:
            imp = 0.0 - np.where(c0 != 0.0, f0 * _log2(np.where(c0 != 0.0, f0, 1.0)), 0.0)
            imp = imp - np.where(c1 != 0.0, f1 * _log2(np.where(c1 != 0.0, f1, 1.0)), 0.0)
    return np.where(t == 0.0, 0.0, imp)


def best_split(hist, nthr, kind, min_instances):
    """hist: int [d][B][2].  Returns (feature, split, gain, left counts, right counts, total
    counts): the first maximum in feature-major then split order."""
    d, B, _ = hist.shape
    tot = hist[0].sum(axis=0).astype(np.float64)
    T = B - 1
    L = np.cumsum(hist[:, :T, :], axis=1).astype(np.float64)  # [d][T][2]
    R = tot[None, None, :] - L
    lc, rc = L[..., 0] + L[..., 1], R[..., 0] + R[..., 1]
    t = lc + rc
    with np.errstate(invalid="ignore", divide="ignore"):
        imp_l, imp_r = impurity(kind, L[..., 0], L[..., 1]), impurity(kind, R[..., 0], R[..., 1])
        gain = float(impurity(kind, tot[0], tot[1])) - (lc / t) * imp_l
        gain = gain - (rc / t) * imp_r
    bad = (lc < min_instances) | (rc < min_instances)
    gain = np.where(bad | (gain < 0.0), INVALID, gain)
    exists = np.arange(T)[None, :] < np.asarray(nthr)[:, None]
    gain = np.where(exists, gain, -np.inf)
    k = int(np.argmax(gain))  # the first of equal maxima
    f, s = divmod(k, T)
    if not exists[f, s]:
        return None
    return f, s, float(gain[f, s]), L[f, s], R[f, s], tot


def _predict_of(c):
    return 1.0 if c[1] > c[0] else 0.0


def train(X, y, impurity_kind="gini", max_depth=5, max_bins=32, min_instances_per_node=1,
          sample_rows=None):
    """The tree as a NODE array ascending by id.  sample_rows: the rows the thresholds come from
    when n > required_samples(max_bins) (a Spark sampler's outcome); every row otherwise."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, d = X.shape
    assert n >= 2 and np.all(np.isfinite(X)) and np.all((y == 0.0) | (y == 1.0))
    B = min(max_bins, n)
    T = B - 1
    S = X if n <= required_samples(max_bins) else X[np.asarray(sample_rows)]
    thr = [thresholds(S[:, f], T) for f in range(d)]
    nthr = [len(t) for t in thr]
    bins = np.stack([np.searchsorted(np.asarray(thr[f]), X[:, f], side="left")
                     for f in range(d)], axis=1)  # thresholds below the value
    lab = (y == 1.0).astype(np.int64)
    key = (np.arange(d)[None, :] * B + bins) * 2 + lab[:, None]

    nodes = [dict(id=1, feature=-1, left=-1, right=-1, threshold=0.0, predict=0.0, impurity=0.0,
                  gain=0.0)]
    active = [(0, np.arange(n))]
    level = 0
    while active:
        nxt = []
        for pos, rows in active:
            hist = np.bincount(key[rows].ravel(), minlength=d * B * 2).reshape(d, B, 2)
            best = best_split(hist, nthr, impurity_kind, min_instances_per_node)
            if level == 0:
                tot = hist[0].sum(axis=0).astype(np.float64)
                nodes[0]["predict"] = _predict_of(tot)
                nodes[0]["impurity"] = float(impurity(impurity_kind, tot[0], tot[1]))
            if best is None or best[2] <= 0.0 or level == max_depth:
                continue
            f, s, gain, Lc, Rc, _ = best
            nd = nodes[pos]
            nd.update(feature=f, threshold=thr[f][s], gain=gain)
            go_left = bins[rows, f] <= s
            for side, c, sub in ((0, Lc, rows[go_left]), (1, Rc, rows[~go_left])):
                imp = float(impurity(impurity_kind, c[0], c[1]))
                child = len(nodes)
                nodes.append(dict(id=2 * nd["id"] + side, feature=-1, left=-1, right=-1,
                                  threshold=0.0, predict=_predict_of(c), impurity=imp, gain=0.0))
                nd["left" if side == 0 else "right"] = child
                if not (level + 1 == max_depth or imp == 0.0):
                    nxt.append((child, sub))
        active = nxt
        level += 1
    out = np.zeros(len(nodes), dtype=NODE)
    for i, nd in enumerate(nodes):
        for k, v in nd.items():
            out[i][k] = v
    return out


def predict(nodes, X):
    """Walk from the root: left iff x[feature] <= threshold (a NaN goes right)."""
    X = np.asarray(X, dtype=np.float64)
    at = np.zeros(X.shape[0], dtype=np.int64)
    while True:
        f = nodes["feature"][at]
        inner = np.nonzero(f >= 0)[0]
        if inner.size == 0:
            break
        a = at[inner]
        with np.errstate(invalid="ignore"):
            left = X[inner, f[inner]] <= nodes["threshold"][a]
        at[inner] = np.where(left, nodes["left"][a], nodes["right"][a])
    return nodes["predict"][at].astype(np.float64)
