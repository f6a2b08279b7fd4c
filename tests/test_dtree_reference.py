"""train_clf=dt off the GPU: the Python restatement of MLlib 1.6.2 DecisionTree
(tests/dtree_reference.py) pinned by hand-worked cases and by the fixtures'
trees, the argument checks of the C ABI that need no device, and the library's host logic
(csrc/dtree_host.h) built into a stand-alone program under AddressSanitizer + UBSan and compared
with the restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import dtree_reference as R
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from conftest import REPO, hexrows

A, B_, C = -1.5, 0.25, 7.0


# ---- thresholds ------------------------------------------------------------------------------
def test_stride_scan_by_hand():
    # stride 50: after a (1 row) and b (2 rows) the count is nearer the target before c joins
    assert R.thresholds([A] * 1 + [B_] * 1 + [C] * 98, 1) == [B_]
    # stride 50: 60 rows of a are nearer 50 than 80 are; the next target, 100, is met exactly by
    # the last value, which is never a threshold
    assert R.thresholds([A] * 60 + [B_] * 20 + [C] * 20, 1) == [A]
    # order of the input does not matter, -0.0 and 0.0 are one value
    assert R.thresholds([0.0, C, -0.0, A], 3) == [A, 0.0, C]


def test_few_distinct_values_are_all_thresholds():
    assert R.thresholds([C, A, C, B_, A, A], 3) == [A, B_, C]
    assert R.thresholds([C, A, C, B_, A, A], 31) == [A, B_, C]
    assert R.thresholds([C] * 9, 31) == [C]


def test_constant_column_never_splits():
    X = np.array([[C, 1.0], [C, 2.0], [C, 3.0], [C, 4.0]])
    t = R.train(X[:, :1], [0, 1, 0, 1])
    assert len(t) == 1 and t[0]["feature"] == -1  # the only split leaves nobody on the right
    t = R.train(X, [0, 0, 1, 1])
    assert t[0]["feature"] == 1 and t[0]["threshold"] == 2.0


# ---- a 4-row tree by hand ----------------------------------------------------------------------
def test_tie_between_features_keeps_the_first():
    # 4 rows, 4 bins: thresholds [1, 2, 3] and [5, 6, 7]; the middle split of either feature
    # separates the classes (gain 0.5), and maxBy keeps feature 0
    X = np.array([[1.0, 5.0], [2.0, 6.0], [3.0, 7.0], [4.0, 8.0]])
    for kind, root_imp in (("gini", 0.5), ("entropy", 1.0)):
        t = R.train(X, [0, 0, 1, 1], kind)
        assert t["id"].tolist() == [1, 2, 3]
        assert (t[0]["feature"], t[0]["threshold"], t[0]["left"], t[0]["right"]) == (0, 2.0, 1, 2)
        assert t[0]["gain"] == root_imp and t[0]["impurity"] == root_imp
        assert t[0]["predict"] == 0.0  # 2 : 2, class 0 on a tie
        # both children are pure: leaves at level 1, long before max_depth 5
        assert t["feature"].tolist()[1:] == [-1, -1] and t["impurity"].tolist()[1:] == [0.0, 0.0]
        assert t["predict"].tolist()[1:] == [0.0, 1.0]
        assert R.predict(t, X).tolist() == [0.0, 0.0, 1.0, 1.0]


def test_tie_between_splits_keeps_the_first():
    # labels 0 1 1 0 over x = 1 2 3 4: the splits at 1 and at 3 both gain 0.5 - 3/4 * 4/9 = 1/6,
    # the split at 2 gains 0; the first wins.  Node 3 (x = 2 3 4, labels 1 1 0): the split at 1 is
    # invalid (nobody left), at 2 gains 4/9 - 2/3 * 1/2 = 1/9, at 3 gains 4/9.
    X = np.array([[1.0], [2.0], [3.0], [4.0]])
    t = R.train(X, [0, 1, 1, 0])
    assert t["id"].tolist() == [1, 2, 3, 6, 7]
    assert t["feature"].tolist() == [0, -1, 0, -1, -1]
    assert t["left"].tolist() == [1, -1, 3, -1, -1] and t["right"].tolist() == [2, -1, 4, -1, -1]
    assert t[0]["threshold"] == 1.0 and t[2]["threshold"] == 3.0
    assert t[0]["gain"] == pytest.approx(1 / 6, rel=1e-15)
    assert t[2]["gain"] == pytest.approx(4 / 9, rel=1e-15)
    assert t[2]["impurity"] == pytest.approx(4 / 9, rel=1e-15)
    assert t["predict"].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]
    Z = [[0.5], [1.0], [1.5], [3.0], [3.5], [np.nan], [np.inf], [-np.inf]]
    assert R.predict(t, Z).tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    # min_instances_per_node 2 leaves the root only the middle split, whose gain is 0: a leaf
    assert len(R.train(X, [0, 1, 1, 0], min_instances_per_node=2)) == 1
    # max_depth 1 stops below the root
    t1 = R.train(X, [0, 1, 1, 0], max_depth=1)
    assert t1["id"].tolist() == [1, 2, 3] and t1["feature"].tolist() == [0, -1, -1]


def test_single_leaf_trees():
    X = np.array([[1.0], [2.0], [3.0], [4.0]])
    t = R.train(X, [0, 1, 1, 1], max_depth=0)
    assert len(t) == 1 and t[0]["feature"] == -1 and t[0]["predict"] == 1.0
    assert t[0]["impurity"] == 1.0 - 0.25 * 0.25 - 0.75 * 0.75
    for lab in (0.0, 1.0):
        t = R.train(X, [lab] * 4)
        assert len(t) == 1 and t[0]["predict"] == lab and t[0]["impurity"] == 0.0
        assert (t[0]["left"], t[0]["right"], t[0]["gain"]) == (-1, -1, 0.0)


# ---- the fixtures' trees -----------------------------------------------------------------------
def _splits(t):
    return {int(n["id"]): (int(n["feature"]), float(n["threshold"]).hex())
            for n in t if n["feature"] >= 0}


def test_fixture_trees(golden_vectors):
    g = golden_vectors["infoTrain"]
    X, y = hexrows(g["features_hex"]), np.array(g["labels"], dtype=np.float64)
    for kind in ("gini", "entropy"):
        t = R.train(X, y, kind)
        assert len(t) == 5
        assert _splits(t) == {1: (43, "0x1.d0100c57eb5b7p-6"), 3: (1, "-0x1.155092b1b5a8ap-5")}
        assert np.array_equal(R.predict(t, X), y)
    g = golden_vectors["DoD_2015_02_g4"]
    X, y = hexrows(g["features_hex"]), np.array(g["labels"], dtype=np.float64)
    t = R.train(X, y, "gini")
    assert len(t) == 9
    assert _splits(t) == {1: (31, "0x1.840ec3c3431b9p-7"), 2: (7, "0x1.500a6b60d152fp-4"),
                          4: (7, "-0x1.0cd2b1a9c8502p-3"), 8: (1, "-0x1.9f9b9114fada9p-5")}
    assert np.array_equal(R.predict(t, X), y)
    t = R.train(X, y, "entropy")
    assert len(t) == 9 and sorted(_splits(t)) == [1, 2, 4, 9]
    assert _splits(t)[2] == (29, "0x1.09b6655db981cp-7")
    assert _splits(t)[9] == (0, "0x1.18e7aa02196afp-4")
    assert np.array_equal(R.predict(t, X), y)


# ---- the C ABI without a device ----------------------------------------------------------------
def test_null_context_is_refused():
    # the first check of both entries, before any device call (the checks that need a context
    # are in tests/test_gpu_dtree.py)
    X, y, out = np.zeros((4, 2)), np.zeros(4), np.zeros(4)
    nodes = np.zeros(7, dtype=R.NODE)
    nodes["feature"] = nodes["left"] = nodes["right"] = -1
    from ctypes import byref, c_int32
    count = c_int32()
    assert fx.lib().eegfx_dtree_train(None, _lib.ptr(X), _lib.ptr(y), 4, 2, 0, 5, 32, 1, 0,
                                      _lib.ptr(nodes), 7, byref(count), 0) == _lib.EEGFX_EINVAL
    assert b"null context" in fx.lib().eegfx_last_error()
    assert fx.lib().eegfx_dtree_predict(None, _lib.ptr(X), 4, 2, _lib.ptr(nodes), 1,
                                        _lib.ptr(out), 0) == _lib.EEGFX_EINVAL


def test_python_node_layout_is_the_headers():
    from eeg_dataanalysispackage_amd import classification as clf
    assert clf.TREE_NODE.itemsize == 48 and clf.TREE_NODE.itemsize == R.NODE.itemsize
    assert [clf.TREE_NODE.fields[k][1] for k in R.NODE.names] == \
        [R.NODE.fields[k][1] for k in R.NODE.names]
    assert {"DecisionTreeClassifier", "dtree_train", "dtree_predict"} <= set(fx.__all__)


# ---- csrc/dtree_host.h under AddressSanitizer + UBSan -------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dtree") / "dtree_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc"),
                    os.path.join(REPO, "tests", "c_abi", "dtree_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("kind", ["gini", "entropy"])
@pytest.mark.parametrize("max_bins,quantum", [(2, None), (4, None), (32, None), (32, 0.25),
                                              (256, None)])
def test_host_logic_matches_the_restatement(host_check, tmp_path, kind, max_bins, quantum):
    rng = np.random.default_rng(max_bins)
    n, d = 70, 3
    X = rng.standard_normal((n, d))
    if quantum:
        X = np.round(X / quantum) * quantum  # duplicates; distinct <= numSplits in places
    X[:, 2] = 3.0 if quantum else X[:, 2]    # and a constant column
    y = (X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        f.write(f"{0 if kind == 'gini' else 1} {max_bins} 1 {n} {d}\n")
        for r in range(n):
            f.write(" ".join(float(v).hex() for v in X[r]) + " " + float(y[r]).hex() + "\n")
    lines = _run(host_check, "split", case)
    T = min(max_bins, n) - 1
    thr = [R.thresholds(X[:, c], T) for c in range(d)]
    for c in range(d):
        assert lines[c].split()[:2] == ["thr", f"{c}:"]
        assert [float.fromhex(v) for v in lines[c].split()[2:]] == thr[c]
    root = R.train(X, y, kind, max_depth=1, max_bins=max_bins)[0]
    assert root["feature"] >= 0
    tag, f_, s_, gain, imp = lines[d].split()
    assert tag == "root" and int(f_) == root["feature"]
    assert thr[int(f_)][int(s_)] == root["threshold"]
    assert float.fromhex(gain).hex() == float(root["gain"]).hex()
    assert float.fromhex(imp).hex() == float(root["impurity"]).hex()


def _growth_case(n, d, what):
    rng = np.random.default_rng(1000 * n + d)
    X = rng.standard_normal((n, d))
    y = (X @ rng.standard_normal(d) + 0.7 * rng.standard_normal(n) > 0).astype(np.float64)
    if what == "constant column":
        X[:, 1] = -2.5
    if what == "one class":
        y[:] = 1.0
    return X, y


@pytest.mark.parametrize("min_instances", [1, 5])
@pytest.mark.parametrize("max_depth", [0, 1, 5])
@pytest.mark.parametrize("kind", ["gini", "entropy"])
@pytest.mark.parametrize("n,d,what", [(300, 4, "plain"), (257, 7, "plain"),
                                      (257, 7, "constant column"), (300, 4, "one class")])
def test_host_growth_matches_the_restatement(host_check, tmp_path, n, d, what, kind, max_depth,
                                             min_instances):
    """dtree::best_split and dtree::grow_node grow a whole tree on the CPU from binned rows (the
    check program counts each node's histogram itself); every node equals the restatement's: the
    leaf rule, the ids 2 id + side, the order the children are appended in."""
    X, y = _growth_case(n, d, what)
    B = 32
    thr = [R.thresholds(X[:, c], B - 1) for c in range(d)]
    bins = np.stack([np.searchsorted(np.asarray(thr[c]), X[:, c], side="left") for c in range(d)],
                    axis=1)
    case = tmp_path / "grow.txt"
    with open(case, "w") as f:
        f.write(f"{0 if kind == 'gini' else 1} {max_depth} {min_instances} {n} {d} {B}\n")
        for t in thr:
            f.write(" ".join([str(len(t))] + [float(v).hex() for v in t]) + "\n")
        for r in range(n):
            f.write(" ".join(str(int(b)) for b in bins[r]) + " " + float(y[r]).hex() + "\n")
    lines = _run(host_check, "grow", case)
    want = R.train(X, y, kind, max_depth=max_depth, max_bins=B,
                   min_instances_per_node=min_instances)
    assert len(lines) == len(want)
    if what != "one class" and max_depth == 5 and min_instances == 1:
        assert len(want) > 7   # a real tree: several levels, leaves above max_depth among them
    for line, nd in zip(lines, want):
        v = line.split()
        assert [int(x) for x in v[:4]] == [int(nd[k]) for k in ("id", "feature", "left", "right")]
        assert [float.fromhex(x).hex() for x in v[4:]] == \
            [float(nd[k]).hex() for k in ("threshold", "predict", "impurity", "gain")]


@pytest.mark.parametrize("rows,d,valid", [
    ([(0, 1, 2), (-1, -1, -1), (-1, -1, -1)], 1, 1),
    ([(-1, -1, -1)], 1, 1),
    ([(0, 1, 3), (-1, -1, -1), (-1, -1, -1)], 1, 0),    # a child past the end
    ([(0, 0, 2), (-1, -1, -1), (-1, -1, -1)], 1, 0),    # a child that is its parent: a cycle
    ([(0, 1, 2), (0, 0, 2), (-1, -1, -1)], 1, 0),       # a child before its parent
    ([(0, -1, 2), (-1, -1, -1), (-1, -1, -1)], 1, 0),   # an inner node without a left child
    ([(1, 1, 2), (-1, -1, -1), (-1, -1, -1)], 1, 0),    # feature >= d
    ([(-2, 1, 2), (-1, -1, -1), (-1, -1, -1)], 1, 0),   # a negative feature that is no leaf mark
    ([(-1, 1, 2), (-1, -1, -1), (-1, -1, -1)], 1, 0),   # a leaf with children
    ([], 1, 0),
])
def test_corrupt_node_arrays_are_refused(host_check, tmp_path, rows, d, valid):
    case = tmp_path / "nodes.txt"
    case.write_text(f"{len(rows)} {d}\n" + "".join("%d %d %d\n" % r for r in rows))
    assert _run(host_check, "nodes", case) == [f"valid {valid}"]
