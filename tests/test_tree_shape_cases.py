"""tests/tree_shape_cases.py off the GPU: every case reaches the path it exists for, asserted on
the Python restatements alone (tests/dtree_reference.py, tests/rforest_reference.py) and on the
launchers' arithmetic as DESIGN.md section 10.3 states it.  A seed or a shape changed later cannot
then empty a case silently: tests/test_gpu_tree_shapes.py compares the device with the
restatements at exactly these inputs."""
import ast
import inspect
import os

import numpy as np
import pytest

import dtree_reference as D
import tree_shape_cases as T


def ids(cases):
    return [c.name for c in cases]


def test_rows_and_probes_are_the_generators_of_test_gpu_dtree():
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_dtree.py")).read()
    theirs = {f.name: f for f in ast.parse(src).body if isinstance(f, ast.FunctionDef)}
    for fn in (T.rows, T.probes):
        ours = ast.parse(inspect.getsource(fn)).body[0]
        assert [ast.dump(s) for s in theirs[fn.__name__].body[1:]] == \
            [ast.dump(s) for s in ours.body[1:]]


def test_case_names_are_distinct():
    cases = [T.A1, T.A2, T.A5, T.A6, T.B2, T.C3] + T.A3 + T.PREDICT_TRAIN + T.B1 + T.B3
    assert len({c.name for c in cases}) == len(cases)


# ---- A: later trips ------------------------------------------------------------------------------
def test_a1_single_tree_past_the_route_stride():
    c = T.A1
    assert c.n > T.ROUTE_ROWS_PER_TRIP and c.d <= 64 and not c.trees
    assert -(-c.n // T.HIST_ROWS_PER_TRIP) == 17      # trips of dt_hist<true,true>
    assert -(-c.n // T.ROUTE_ROWS_PER_TRIP) == 2      # trips of rf_route
    assert 0 < T.sample_rows(c).size < c.n
    for kind in T.KINDS:
        assert len(T.restated(c, kind)) >= 7
    assert len(T.restated(c, "gini")) == 15


def test_a2_weighted_single_tree_on_the_same_rows():
    c = T.A2
    assert T.inputs(c)[0] is T.inputs(T.A1)[0]
    assert c.trees == 1 and T.features_per_node(c) == 2 < c.d      # not the plain tree
    assert np.all(T.bag(c) == 1)
    for kind in T.KINDS:
        nodes, off, drawn, _ = T.restated(c, kind)
        assert len(nodes) >= 7 and off.tolist() == [0, len(nodes)]
        assert any(feats != [0, 1] for feats in drawn.values())


@pytest.mark.parametrize("c", T.A3, ids=ids(T.A3))
def test_a3_forest_histograms_take_a_second_trip(c):
    assert T.HIST_ROWS_PER_TRIP < c.n <= 2 * T.HIST_ROWS_PER_TRIP
    k = T.features_per_node(c)
    counters = k * c.max_bins * 2
    # rf_hist<true,true>, <true,false>, <false,false>
    assert (c.d <= 64, counters <= T.LDS_COUNTERS) == \
        {3: (True, True), 65: (False, True), 130: (False, False)}[c.d]
    assert (T.sample_rows(c) is None) == (c.max_bins == 256)
    W = T.bag(c)[:, T.HIST_ROWS_PER_TRIP:]
    assert (W >= 3).any() and (W == 0).any()
    if c.data == "sixteenths":
        X = T.inputs(c)[0]
        assert max(len(np.unique(X[:, f])) for f in range(c.d)) < c.max_bins
    for kind in T.KINDS:
        forest = T.restated(c, kind)
        assert all(T.tree_of(forest, t)[0]["feature"] >= 0 for t in range(c.trees))


@pytest.mark.parametrize("c", T.PREDICT_TRAIN, ids=ids(T.PREDICT_TRAIN))
def test_a4_predictions_past_the_grid_cap_see_both_classes(c):
    assert T.PREDICT_N > T.PREDICT_ROWS_PER_TRIP
    for kind in T.KINDS:
        late = T.restated_predictions(c, kind)[T.PREDICT_ROWS_PER_TRIP:]
        assert late.size == T.PREDICT_N - T.PREDICT_ROWS_PER_TRIP
        assert (late == 0.0).any() and (late == 1.0).any()
        m = T.restated(c, kind)
        assert len(m[0] if c.trees else m) > 7


def test_a5_more_trees_than_grid_y():
    c = T.A5
    assert c.trees > T.TREES_PER_TRIP
    for kind in T.KINDS:
        forest = T.restated(c, kind)
        assert forest[3][0] == c.trees     # every root leaves the queue in one group
        assert any(len(T.tree_of(forest, t)) > 1 for t in range(T.TREES_PER_TRIP, c.trees))
        # and a later group holds trees on both sides of the cap: its route takes the trip too
        assert any(len(T.tree_of(forest, t)) > 3 for t in range(T.TREES_PER_TRIP, c.trees))


def test_a6_gathered_sample_past_the_grid_cap():
    c = T.A6
    kept = T.sample_rows(c)
    assert c.device and 0 < kept.size < c.n and kept.size * c.d > T.GATHER_PER_TRIP
    assert len(T.restated(c, "gini")) >= 3


# ---- B: exact boundaries -------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.B1, ids=ids(T.B1))
def test_b1_node_sizes_around_the_lds_bound(c):
    assert c.n >= c.max_bins and T.features_per_node(c) == c.d
    counters = c.d * c.max_bins * 2
    want = {(64, 32): 4096, (63, 32): 4032, (64, 256): T.LDS_COUNTERS,
            (128, 128): T.LDS_COUNTERS, (128, 129): T.LDS_COUNTERS + 256}
    assert counters == want[(c.d, c.max_bins)]
    for kind in T.KINDS:
        m = T.restated(c, kind)
        trees = [T.tree_of(m, t) for t in range(c.trees)] if c.trees else [m]
        assert all(t[0]["feature"] >= 0 for t in trees)
        assert any(len(t) > 3 for t in trees)      # a level below the root gets histograms


def test_b2_a_level_fills_lds():
    c = T.B2
    per_launch = T.LDS_COUNTERS // (c.d * c.max_bins * 2)
    assert per_launch == 128 and per_launch * c.d * c.max_bins * 2 == T.LDS_COUNTERS
    levels = T.active_per_level(T.restated(c, "gini"), c.max_depth)
    assert {lv: int(levels[lv]) for lv in T.B2_LEVELS} == T.B2_LEVELS
    for kind in T.KINDS:
        assert T.active_per_level(T.restated(c, kind), c.max_depth).max() >= per_launch


@pytest.mark.parametrize("c", T.B3, ids=ids(T.B3))
def test_b3_pair_loop_edges(c):
    k = T.features_per_node(c)
    assert (c.d, c.trees, k, c.trees * k) in ((64, 8, 8, 64), (25, 13, 5, 65))
    assert c.trees <= T.LDS_COUNTERS // (k * c.max_bins * 2)      # the roots: one launch
    t, j = divmod(c.pair, k)
    assert c.pair == c.trees * k - 1 and c.pair in (63, 64)      # the last lane that is in
    f = T.decisive_feature(c)
    for kind in T.KINDS:
        forest = T.restated(c, kind)
        assert forest[3][0] == c.trees
        assert forest[2][(t, 1)][j] == f
        root = T.tree_of(forest, t)[0]
        assert root["feature"] == f and root["gain"] > 0.0


# ---- C: decisive lanes, bins and list positions ----------------------------------------------------
def pure_root(tree, X, f, s):
    root = tree[0]
    return (root["feature"] == f and root["threshold"] == D.thresholds(X[:, f], 31)[s]
            and len(tree) == 3 and np.all(tree["impurity"][1:] == 0.0))


@pytest.mark.parametrize("d,f", [(d, f) for d, fs in T.C1_FEATURES.items() for f in fs])
def test_c1_the_chosen_candidate_wins(d, f):
    for s in T.C_SPLITS:
        c = T.c1(d, f, s)
        X, y = T.inputs(c)
        assert len(D.thresholds(X[:, f], 31)) == 31 and 0.0 < y.mean() < 1.0
        for kind in T.KINDS:
            assert pure_root(T.restated(c, kind), X, f, s), (s, kind)


@pytest.mark.parametrize("d,f", [(d, f) for d, fs in T.C2_FEATURES.items() for f in fs])
def test_c2_every_root_picks_the_feature(d, f):
    c = T.c2(d, f)
    for kind in T.KINDS:
        forest = T.restated(c, kind)
        for t in range(c.trees):
            tree = T.tree_of(forest, t)
            assert tree[0]["feature"] == f and np.all(tree["impurity"][1:] == 0.0)


def test_c3_the_feature_wins_from_every_list_position():
    c = T.C3
    assert T.features_per_node(c) == 7 and c.parts == 2 and T.FOREST_SEED == 12345
    for kind in T.KINDS:
        forest = T.restated(c, kind)
        assert forest[3][0] == c.trees
        positions = []
        for t in range(c.trees):
            feats = forest[2][(t, 1)]
            assert feats == T.root_lists(c)[t]
            if c.f in feats:
                assert T.tree_of(forest, t)[0]["feature"] == c.f
                positions.append(feats.index(c.f))
        assert sorted(positions) == T.C3_POSITIONS and set(positions) == set(range(7))
