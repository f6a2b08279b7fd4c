"""MLlib 1.6.2 RandomForest as Classification/RandomForestClassifier.java:101-136 runs it (two
classes, continuous features), restated in Python from DESIGN.md section 10.2.  Not a test module:
tests/test_rforest_reference.py pins it by hand-worked cases and tests/test_gpu_rforest.py
compares the device with it, exactly.  It shares no code with the product: the thresholds, the
impurities and the per-node rule are tests/dtree_reference.py's, java.util.Random and
XORShiftRandom are oracle/mllib_logreg.py's (pinned by tests/test_spark_sample.py).
"""
from collections import deque

import numpy as np

import dtree_reference as D
from oracle.mllib_logreg import JavaRandom, XORShiftRandom

NODE = D.NODE
M32 = 0xFFFFFFFF
SUBSETS = ("auto", "all", "sqrt", "log2", "onethird")
MAX_MEMORY = 256 * 2 ** 20   # Strategy.maxMemoryInMB
EXP_M1 = float.fromhex("0x1.78b56362cef38p-2")   # exp(-1), correctly rounded


class Well19937c:
    """org.apache.commons.math3.random.Well19937c: 624 32-bit words and an index."""

    def __init__(self, seed):
        seed &= (1 << 64) - 1
        v = [seed >> 32, seed & M32]
        for i in range(2, 624):
            w = v[i - 2]
            l = w - (1 << 32) if w >> 31 else w        # (long) v[i - 2], sign-extended
            v.append((1812433253 * (l ^ (l >> 30)) + i) & M32)   # >> on a Python int is arithmetic
        self.v, self.index = v, 0

    def next(self, bits):
        v, i = self.v, self.index
        m1, m2 = (i + 623) % 624, (i + 622) % 624
        v0, a, b, c = v[i], v[(i + 70) % 624], v[(i + 179) % 624], v[(i + 449) % 624]
        z0 = (0x80000000 & v[m1]) ^ (0x7FFFFFFF & v[m2])
        z1 = (v0 ^ (v0 << 25) ^ a ^ (a >> 27)) & M32
        z2 = (b >> 9) ^ c ^ (c >> 1)
        z3 = z1 ^ z2
        z4 = (z0 ^ z1 ^ (z1 << 9) ^ z2 ^ (z2 << 21) ^ z3 ^ (z3 >> 21)) & M32
        v[m1], v[i] = z3, z4
        v[m2] &= 0x80000000
        self.index = m1
        z4 ^= (z4 << 7) & 0xe46e1700
        z4 ^= (z4 << 15) & 0x9b868000
        return (z4 & M32) >> (32 - bits)

    def next_double(self):
        return ((self.next(26) << 26) | self.next(26)) * 2.0 ** -52


def poisson1(rng):
    """PoissonDistribution(1.0).sample()."""
    n, r = 0, 1.0
    while n < 1000:
        r *= rng.next_double()
        if r >= EXP_M1:
            n += 1
        else:
            return n
    return n


def bag(n, num_trees, num_partitions, seed):
    """BaggedPoint.convertToBaggedRDD: weights [num_trees][n].  One tree: all 1.  Otherwise slice p
    of the rows draws row by row, tree by tree, from its own sampler seeded seed + p + 1."""
    w = np.ones((num_trees, n), dtype=np.int64)
    if num_trees == 1:
        return w
    for p in range(num_partitions):
        a, b = p * n // num_partitions, (p + 1) * n // num_partitions
        rng = Well19937c(seed + p + 1)
        for r in range(a, b):
            for t in range(num_trees):
                w[t, r] = poisson1(rng)
    return w


def features_per_node(subset, num_trees, d):
    assert subset in SUBSETS
    if subset == "auto":
        subset = "all" if num_trees == 1 else "sqrt"
    if subset == "all":
        return d
    if subset == "sqrt":       # ceil(sqrt d), in integers
        return next(k for k in range(d + 1) if k * k >= d)
    if subset == "log2":       # max(1, ceil(log2 d)), in integers
        return max(1, (d - 1).bit_length())
    return -(-d // 3)          # onethird


def reservoir(d, k, seed):
    """SamplingUtils.reservoirSampleAndCount over 0..d-1: k features in reservoir order."""
    res = list(range(k))
    if k >= d:
        return res
    rand = XORShiftRandom(seed)
    l = k
    for item in range(k, d):
        l += 1
        j = int(rand.next_double() * l)
        if j < k:
            res[j] = item
    return res


def next_group(queue, rng, d, k, subsample, node_bytes):
    """RandomForest.selectNodesToSplit: [(queued node, subset or None)].  Every node looked at
    draws its subset, the one that does not fit included: it stays queued."""
    group, mem = [], 0
    while queue and mem < MAX_MEMORY:
        subset = reservoir(d, k, rng.next_long()) if subsample else None
        if mem + node_bytes <= MAX_MEMORY:
            group.append((queue.popleft(), subset))
        mem += node_bytes
    return group


def _best(hist, feats, nthr, kind, min_instances):
    """D.best_split over the node's feature list: hist [k][B][2] in list order."""
    best = D.best_split(hist, [nthr[f] for f in feats], kind, min_instances)
    if best is None:
        return None
    return (feats[best[0]],) + best[1:]


def train(X, y, impurity_kind="gini", max_depth=5, max_bins=32, min_instances_per_node=1,
          num_trees=100, feature_subset="auto", seed=12345, num_partitions=1, sample_rows=None,
          weights=None):
    """(nodes, tree_offsets, subsets, group sizes): the trees concatenated (children relative to
    the tree), the offsets, {(tree, node id): the feature list its split was chosen from}, and the
    number of nodes of each group that left the queue.  weights: the bag, when the caller has
    drawn it already."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, d = X.shape
    assert n >= 2 and np.all(np.isfinite(X)) and np.all((y == 0.0) | (y == 1.0))
    B = min(max_bins, n)
    T = B - 1
    S = X if n <= D.required_samples(max_bins) else X[np.asarray(sample_rows)]
    thr = [D.thresholds(S[:, f], T) for f in range(d)]
    nthr = [len(t) for t in thr]
    bins = np.stack([np.searchsorted(np.asarray(thr[f]), X[:, f], side="left")
                     for f in range(d)], axis=1)
    lab = (y == 1.0).astype(np.int64)
    W = bag(n, num_trees, num_partitions, seed) if weights is None else np.asarray(weights)
    k = features_per_node(feature_subset, num_trees, d)
    subsample = k < d
    node_bytes = B * 2 * (k if subsample else d) * 8
    rng = JavaRandom(seed)

    def leaf(i, predict=0.0, imp=0.0):
        return dict(id=i, feature=-1, left=-1, right=-1, threshold=0.0, predict=predict,
                    impurity=imp, gain=0.0)

    trees = [[leaf(1)] for _ in range(num_trees)]
    drawn, sizes = {}, []
    # a queued node: (tree, position in the tree, level, its rows)
    queue = deque((t, 0, 0, np.nonzero(W[t])[0]) for t in range(num_trees))
    while queue:
        group = next_group(queue, rng, d, k, subsample, node_bytes)
        assert group
        sizes.append(len(group))
        children = []   # (tree, order in the group, [queued children])
        for order, ((t, pos, level, rows), subset) in enumerate(group):
            feats = subset if subsample else list(range(d))
            nodes = trees[t]
            nd = nodes[pos]
            drawn[(t, nd["id"])] = feats
            key = (np.arange(len(feats))[None, :] * B + bins[rows][:, feats]) * 2 + lab[rows, None]
            hist = np.bincount(key.ravel(), weights=np.repeat(W[t, rows], len(feats)),
                               minlength=len(feats) * B * 2)
            hist = np.rint(hist).astype(np.int64).reshape(len(feats), B, 2)
            tot = hist[0].sum(axis=0).astype(np.float64)
            if level == 0:
                nd["predict"] = D._predict_of(tot)
                nd["impurity"] = float(D.impurity(impurity_kind, tot[0], tot[1]))
            best = _best(hist, feats, nthr, impurity_kind, min_instances_per_node)
            if best is None or best[2] <= 0.0 or level == max_depth:
                continue
            f, s, gain, Lc, Rc, _ = best
            nd.update(feature=f, threshold=thr[f][s], gain=gain)
            go_left = bins[rows, f] <= s
            queued = []
            for side, c, sub in ((0, Lc, rows[go_left]), (1, Rc, rows[~go_left])):
                imp = float(D.impurity(impurity_kind, c[0], c[1]))
                child = len(nodes)
                nodes.append(leaf(2 * nd["id"] + side, D._predict_of(c), imp))
                nd["left" if side == 0 else "right"] = child
                if not (level + 1 == max_depth or imp == 0.0):
                    queued.append((t, child, level + 1, sub))
            children.append((t, order, queued))
        # ascending tree, a tree's nodes in group order, left then right
        for _, _, queued in sorted(children, key=lambda c: (c[0], c[1])):
            queue.extend(queued)
    offsets = np.zeros(num_trees + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(t) for t in trees])
    out = np.zeros(int(offsets[-1]), dtype=NODE)
    i = 0
    for nodes in trees:
        for nd in nodes:
            for name, v in nd.items():
                out[i][name] = v
            i += 1
    return out, offsets, drawn, sizes


def predict(nodes, offsets, X):
    """RandomForestModel.predict: 1.0 iff more trees vote 1 than 0; a tie is 0.0."""
    X = np.asarray(X, dtype=np.float64)
    T = len(offsets) - 1
    ones = np.zeros(X.shape[0], dtype=np.int64)
    for t in range(T):
        ones += D.predict(nodes[offsets[t]:offsets[t + 1]], X) == 1.0
    return (ones > T - ones).astype(np.float64)


def votes(nodes, offsets, X):
    """The number of trees that vote 1 for each row."""
    X = np.asarray(X, dtype=np.float64)
    return sum((D.predict(nodes[offsets[t]:offsets[t + 1]], X) == 1.0).astype(np.int64)
               for t in range(len(offsets) - 1))
