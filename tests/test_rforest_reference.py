"""train_clf=rf off the GPU: the Python restatement of MLlib 1.6.2 RandomForest
(tests/rforest_reference.py) pinned by the draws the contract states and by
hand-worked cases, eegfx_poisson_bag against it, the argument checks of the C ABI that need no
device, and the library's host logic (csrc/rforest_host.h) built into a stand-alone program under
AddressSanitizer + UBSan and compared with the restatement."""
import os
import subprocess
from collections import deque
from ctypes import byref, c_int32

import numpy as np
import pytest

import rforest_reference as R
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd import classification as clf
from oracle.mllib_logreg import JavaRandom, XORShiftRandom
from conftest import REPO

BAG_CASES = [(1, 1, 1), (7, 3, 1), (65, 2, 4), (1000, 100, 16), (10, 3, 16)]
SUBSET_CODES = {"auto": 0, "all": 1, "sqrt": 2, "log2": 3, "onethird": 4}


@pytest.fixture(scope="module")
def bags():
    """The restatement's bag of every case, drawn once."""
    return {c: R.bag(c[0], c[1], c[2], 12345) for c in BAG_CASES}


# ---- the sampler ---------------------------------------------------------------------------------
def test_the_twenty_draws_of_the_contract():
    rng = R.Well19937c(12345 + 0 + 1)
    draws = [R.poisson1(rng) for _ in range(100000)]
    assert draws[:20] == [4, 0, 1, 1, 0, 0, 2, 3, 1, 1, 0, 1, 2, 1, 1, 1, 0, 1, 0, 5]
    assert round(float(np.mean(draws)), 5) == 1.00385 and max(draws) == 8


def test_seed_words_are_sign_extended():
    # a seed whose low word has its top bit set: v[3] comes from (long) v[1] < 0
    rng = R.Well19937c(0x80000001)
    assert rng.v[0] == 0 and rng.v[1] == 0x80000001
    l = 0x80000001 - (1 << 32)
    assert rng.v[3] == (1812433253 * (l ^ (l >> 30)) + 3) & 0xFFFFFFFF
    assert rng.v[3] != (1812433253 * (0x80000001 ^ (0x80000001 >> 30)) + 3) & 0xFFFFFFFF


@pytest.mark.parametrize("case", BAG_CASES)
def test_poisson_bag_matches_restatement(bags, case):
    n, trees, P = case
    got = clf.poisson_bag(n, trees, P, 12345)
    assert got.dtype == np.uint8 and got.shape == (trees, n)
    assert np.array_equal(got, bags[case])
    if trees == 1:
        assert np.all(got == 1)   # no sampler
    if case == (7, 3, 1):
        # one slice: row by row, tree by tree from the sampler seeded 12345 + 0 + 1
        assert got.T.ravel().tolist()[:20] == [4, 0, 1, 1, 0, 0, 2, 3, 1, 1, 0, 1, 2, 1, 1, 1, 0, 1,
                                               0, 5]


def test_poisson_bag_does_not_depend_on_the_thread_count(bags):
    # the library draws the slices on as many threads as the process may run on
    allowed = os.sched_getaffinity(0)
    try:
        os.sched_setaffinity(0, {min(allowed)})
        one = clf.poisson_bag(1000, 100, 16, 12345)
    finally:
        os.sched_setaffinity(0, allowed)
    assert np.array_equal(one, bags[(1000, 100, 16)])
    assert np.array_equal(clf.poisson_bag(1000, 100, 16, 12345), one)


def test_poisson_bag_argument_checks():
    w = np.zeros(8, dtype=np.uint8)
    bag = fx.lib().eegfx_poisson_bag
    assert bag(4, 2, 1, 0, _lib.ptr(w)) == _lib.EEGFX_OK
    assert bag(-1, 2, 1, 0, _lib.ptr(w)) == _lib.EEGFX_EINVAL
    assert bag(4, 0, 1, 0, _lib.ptr(w)) == _lib.EEGFX_EINVAL
    assert bag(4, 2, 0, 0, _lib.ptr(w)) == _lib.EEGFX_EINVAL
    assert bag(4, 2, 1, 0, None) == _lib.EEGFX_EINVAL
    assert bag(0, 2, 1, 0, _lib.ptr(w)) == _lib.EEGFX_OK


# ---- features per node, the reservoir --------------------------------------------------------------
def test_features_per_node():
    want = {1: (1, 1, 1, 1), 2: (2, 2, 1, 1), 3: (3, 2, 2, 1), 4: (4, 2, 2, 2), 48: (48, 7, 6, 16),
            65: (65, 9, 7, 22), 1024: (1024, 32, 10, 342)}   # all, sqrt, log2, onethird
    for d, row in want.items():
        for name, k in zip(("all", "sqrt", "log2", "onethird"), row):
            assert R.features_per_node(name, 3, d) == k, (d, name)
            assert R.features_per_node(name, 1, d) == k, (d, name)
        assert R.features_per_node("auto", 1, d) == row[0]   # one tree: all
        assert R.features_per_node("auto", 2, d) == row[1]   # a forest: sqrt


def test_reservoir_by_hand():
    assert R.reservoir(5, 5, 77) == [0, 1, 2, 3, 4]   # k = d: no draw
    assert R.reservoir(1, 1, 77) == [0]
    # d = 3, k = 2: item 2 arrives with l = 3 and lands at j = (long)(u * 3) when j < 2
    seen = set()
    for seed in range(12):
        u = XORShiftRandom(seed).next_double()
        want = [[2, 1], [0, 2], [0, 1]][int(u * 3)]
        assert R.reservoir(3, 2, seed) == want
        seen.add(tuple(want))
    assert len(seen) == 3   # the seeds reach every outcome
    # the subset keeps reservoir order: it is not sorted
    assert any(R.reservoir(48, 7, s) != sorted(R.reservoir(48, 7, s)) for s in range(4))


def test_a_node_that_does_not_fit_stays_queued_and_draws_again():
    # on paper: 2^20 bins, 10 of 100 features: 2^20 * 2 * 10 * 8 = 160 MB a node, over half of
    # 256 MB.  Three queued nodes leave one per group, and the second and the third draw twice.
    node_bytes = 2 ** 20 * 2 * 10 * 8
    assert 2 * node_bytes > R.MAX_MEMORY >= node_bytes
    queue, rng = deque([("a",), ("b",), ("c",)]), JavaRandom(12345)
    groups = []
    while queue:
        groups.append(R.next_group(queue, rng, 100, 10, True, node_bytes))
    assert [[n for n, _ in g] for g in groups] == [[("a",)], [("b",)], [("c",)]]
    seeds = JavaRandom(12345)
    draws = [R.reservoir(100, 10, seeds.next_long()) for _ in range(5)]
    assert len({tuple(d) for d in draws}) == 5
    # a: draw 0; b: draw 1 is spent when it does not fit, draw 2 counts; c: draw 3 spent, draw 4
    assert [g[0][1] for g in groups] == [draws[0], draws[2], draws[4]]
    # small nodes leave together, each with the next draw
    queue, rng = deque([("a",), ("b",), ("c",)]), JavaRandom(12345)
    g = R.next_group(queue, rng, 100, 10, True, 5120)
    assert [s for _, s in g] == draws[:3] and not queue


# ---- a forest on a three-row toy -------------------------------------------------------------------
def test_toy_forest_by_hand():
    X = np.array([[1.0, 5.0], [2.0, 5.0], [3.0, 5.0]])
    y = [0.0, 1.0, 1.0]
    # one tree, auto: the decision tree itself
    import dtree_reference as D
    nodes, off, drawn, sizes = R.train(X, y, num_trees=1)
    want = D.train(X, y)
    assert nodes.tobytes() == want.tobytes() and off.tolist() == [0, len(want)]
    assert drawn[(0, 1)] == [0, 1] and sizes[0] == 1
    # two trees with stated weights; "sqrt" of 2 features is 2: no subsets, no draw.  Tree 0 sees
    # rows 0 and 2 (weights 2, 1): x <= 1 separates them, gain = 4/9.  Tree 1 sees row 1 alone:
    # a pure root that votes 1.
    W = np.array([[2, 0, 1], [0, 3, 0]])
    nodes, off, drawn, sizes = R.train(X, y, num_trees=2, feature_subset="sqrt", weights=W)
    assert off.tolist() == [0, 3, 4] and sizes == [2]
    assert nodes["id"].tolist() == [1, 2, 3, 1]
    assert nodes["feature"].tolist() == [0, -1, -1, -1]
    assert nodes[0]["threshold"] == 1.0 and nodes[0]["gain"] == pytest.approx(4 / 9, rel=1e-15)
    assert nodes[0]["predict"] == 0.0 and nodes[3]["predict"] == 1.0 and nodes[3]["impurity"] == 0.0
    assert (nodes[0]["left"], nodes[0]["right"]) == (1, 2)   # relative to the tree
    # votes: row 0 gets (0, 1): a tie, 0.0; rows 1 and 2 get (1, 1)
    assert R.votes(nodes, off, X).tolist() == [1, 2, 2]
    assert R.predict(nodes, off, X).tolist() == [0.0, 1.0, 1.0]
    # a tree whose weights are all 0: a leaf that predicts 0 with impurity 0
    W = np.array([[0, 0, 0], [1, 1, 1]])
    nodes, off, _, _ = R.train(X, y, num_trees=2, feature_subset="all", weights=W)
    assert off[1] == 1 and nodes[0]["feature"] == -1
    assert (nodes[0]["predict"], nodes[0]["impurity"]) == (0.0, 0.0)


def test_children_enter_the_queue_by_ascending_tree():
    # 48 features, sqrt: every node draws.  The draws of level 1 go to tree 0's children first,
    # then tree 1's, whatever order the roots were split in.
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 48))
    y = (X[:, 0] + X[:, 1] > 0).astype(np.float64)
    nodes, off, drawn, sizes = R.train(X, y, num_trees=3, max_depth=2, num_partitions=2)
    assert sizes[0] == 3
    seeds = JavaRandom(12345)
    order = [(t, 1) for t in range(3)]
    for t in range(3):
        tree = nodes[off[t]:off[t + 1]]
        if tree[0]["feature"] >= 0:
            order += [(t, int(tree[c]["id"])) for c in (tree[0]["left"], tree[0]["right"])
                      if tree[c]["impurity"] != 0.0]
    assert len(order) > 3
    for key in order:
        assert drawn[key] == R.reservoir(48, 7, seeds.next_long()), key


# ---- the C ABI without a device --------------------------------------------------------------------
def test_null_context_is_refused():
    X, y, out = np.zeros((4, 2)), np.zeros(4), np.zeros(4)
    nodes = np.zeros(7, dtype=R.NODE)
    nodes["feature"] = nodes["left"] = nodes["right"] = -1
    off = np.array([0, 1], dtype=np.int32)
    count = c_int32()
    assert fx.lib().eegfx_rforest_train(None, _lib.ptr(X), _lib.ptr(y), 4, 2, 0, 5, 32, 1, 1, 0,
                                        12345, 1, 0, _lib.ptr(nodes), 7, _lib.ptr(off),
                                        byref(count), 0) == _lib.EEGFX_EINVAL
    assert b"null context" in fx.lib().eegfx_last_error()
    assert fx.lib().eegfx_rforest_predict(None, _lib.ptr(X), 4, 2, _lib.ptr(nodes), _lib.ptr(off),
                                          1, _lib.ptr(out), 0) == _lib.EEGFX_EINVAL


def test_python_surface():
    assert {"RandomForestClassifier", "rforest_train", "rforest_predict",
            "poisson_bag"} <= set(fx.__all__)
    assert clf.FEATURE_SUBSETS == SUBSET_CODES
    assert issubclass(fx.RandomForestClassifier, fx.DecisionTreeClassifier)
    c = fx.RandomForestClassifier(context=object())
    assert c.num_partitions is None and c.split_seed == 0
    with pytest.raises(RuntimeError):
        c.predict(np.zeros((1, 2)))
    with pytest.raises(ValueError):
        clf.rforest_train(None, np.zeros((4, 2)), np.zeros(4), feature_subset="half")
    with pytest.raises(ValueError):
        clf.rforest_predict(None, np.zeros((4, 2)), np.zeros(3, dtype=R.NODE), [0, 2])


# ---- csrc/rforest_host.h under AddressSanitizer + UBSan ---------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rforest") / "rforest_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-pthread", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc"),
                    os.path.join(REPO, "tests", "c_abi", "rforest_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("threads", [1, 3, 16])
@pytest.mark.parametrize("case", BAG_CASES)
def test_host_bag_matches_the_restatement(host_check, bags, case, threads):
    n, trees, P = case
    lines = _run(host_check, "bag", n, trees, P, 12345, threads)
    assert len(lines) == trees
    for t, line in enumerate(lines):
        w, total = line.split("=")
        assert [int(v) for v in w.split()] == bags[case][t].tolist()
        assert int(total) == int(bags[case][t].sum())


def test_host_bag_with_a_negative_seed(host_check):
    lines = _run(host_check, "bag", 9, 2, 2, -7, 2)
    want = R.bag(9, 2, 2, -7)
    assert [[int(v) for v in l.split("=")[0].split()] for l in lines] == want.tolist()


def test_host_features_and_reservoir(host_check):
    for d in (1, 2, 3, 4, 48, 65, 1024):
        for name, code in SUBSET_CODES.items():
            for trees in (1, 3):
                assert _run(host_check, "fpn", code, trees, d) == \
                    [str(R.features_per_node(name, trees, d))]
    assert _run(host_check, "fpn", 5, 3, 48) == ["-1"] and _run(host_check, "fpn", -1, 3, 48) == ["-1"]
    for d, k, seed in ((3, 2, 0), (3, 2, 5), (5, 5, 1), (48, 7, 12345), (48, 7, -3), (1024, 32, 9),
                       (130, 1, 2)):
        assert [int(v) for v in _run(host_check, "reservoir", d, k, seed)[0].split()] == \
            R.reservoir(d, k, seed)


def test_host_groups_match_the_restatement(host_check):
    for d, k, node_bytes, trees in ((100, 10, 2 ** 20 * 2 * 10 * 8, 3), (100, 10, 5120, 3),
                                    (48, 7, 100 * 2 ** 20, 5), (48, 48, 300, 4)):
        queue, rng = deque(range(trees)), JavaRandom(12345)
        want = []
        while queue:
            g = R.next_group(queue, rng, d, k, k < d, node_bytes)
            want.append(" ".join(f"{t}:" + ",".join(str(f) for f in (s or [])) for t, s in g))
        got = [l.strip() for l in _run(host_check, "group", d, k, node_bytes, trees, 12345)]
        assert got == want, (d, k, node_bytes)
    assert len(want) == 1   # the last case: no subsets, one group


@pytest.mark.parametrize("kind", ["gini", "entropy"])
@pytest.mark.parametrize("feats", [[4, 0, 2], [0, 1, 2, 3, 4], [3], [2, 2]])
def test_host_split_over_a_feature_list(host_check, tmp_path, kind, feats):
    rng = np.random.default_rng(len(feats))
    n, d = 70, 5
    X = np.round(rng.standard_normal((n, d)) * 4) / 4
    X[:, 2] = 3.0   # a constant column: no split
    y = (X[:, 0] + 0.5 * X[:, 4] + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    w = rng.integers(0, 4, n)
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        f.write(f"{0 if kind == 'gini' else 1} 32 1 {n} {d} {len(feats)}\n")
        f.write(" ".join(str(v) for v in feats) + "\n")
        for r in range(n):
            f.write(" ".join(float(v).hex() for v in X[r]) + f" {float(y[r]).hex()} {w[r]}\n")
    lines = _run(host_check, "split", case)
    import dtree_reference as D
    B = 32
    thr = [D.thresholds(X[:, c], B - 1) for c in range(d)]
    bins = np.stack([np.searchsorted(np.asarray(thr[c]), X[:, c], side="left") for c in range(d)],
                    axis=1)
    key = (np.arange(len(feats))[None, :] * B + bins[:, feats]) * 2 + (y == 1.0)[:, None]
    hist = np.bincount(key.ravel().astype(np.int64), weights=np.repeat(w, len(feats)),
                       minlength=len(feats) * B * 2).astype(np.int64).reshape(len(feats), B, 2)
    best = R._best(hist, feats, [len(t) for t in thr], kind, 1)
    tag, f_, s_, gain, imp = lines[0].split()
    tot = hist[0].sum(axis=0).astype(np.float64)
    assert float.fromhex(imp).hex() == float(D.impurity(kind, tot[0], tot[1])).hex()
    if best is None:
        assert int(f_) == -1
    else:
        assert (int(f_), int(s_)) == (best[0], best[1])
        assert float.fromhex(gain).hex() == float(best[2]).hex()
    if feats == [0, 1, 2, 3, 4]:
        assert lines[1] == "same 1"   # the identity list is dtree::best_split's choice


LEAF, SPLIT = (-1, -1, -1), (0, 1, 2)


@pytest.mark.parametrize("offsets,rows,d,valid", [
    ([0, 3, 4], [SPLIT, LEAF, LEAF, LEAF], 1, 1),
    ([0, 1], [LEAF], 1, 1),
    ([0, 1, 4], [LEAF, SPLIT, LEAF, LEAF], 1, 1),      # children are relative to the tree
    ([1, 3, 4], [SPLIT, LEAF, LEAF, LEAF], 1, 0),      # the offsets do not start at 0
    ([0, 3, 3], [SPLIT, LEAF, LEAF, LEAF], 1, 0),      # an empty tree
    ([0, 3, 2], [SPLIT, LEAF, LEAF, LEAF], 1, 0),      # descending offsets
    ([0, -1, 4], [SPLIT, LEAF, LEAF, LEAF], 1, 0),     # a negative offset
    ([0, 2, 4], [SPLIT, LEAF, LEAF, LEAF], 1, 0),      # a child past its tree (inside the array)
    ([0, 3, 4], [(1, 1, 2), LEAF, LEAF, LEAF], 1, 0),  # feature >= d
    ([0, 3, 4], [SPLIT, LEAF, LEAF, (-1, 0, 0)], 1, 0),   # a leaf with children, in the last tree
    ([0, 3, 4], [SPLIT, (0, 0, 2), LEAF, LEAF], 1, 0),    # a child before its parent
    ([0, 3], [SPLIT, LEAF, LEAF], 1, 1),
    ([0, 2], [SPLIT, LEAF], 1, 0),                        # truncated: the right child is cut off
])
def test_corrupt_forests_are_refused(host_check, tmp_path, offsets, rows, d, valid):
    case = tmp_path / "forest.txt"
    case.write_text(f"{len(offsets) - 1} {d}\n" + " ".join(str(o) for o in offsets) +
                    f"\n{len(rows)}\n" + "".join("%d %d %d\n" % r for r in rows))
    assert _run(host_check, "forest", case) == [f"valid {valid}"]
