"""The tree kernels (csrc/dtree.hip, csrc/rforest.hip, csrc/hist_lds.h) at the shapes of
tests/tree_shape_cases.py: later trips of the capped grid-stride loops (A), the exact boundaries of
the histogram dispatch (B), and labels that make one chosen lane, bin end or feature-list position
decide the split (C); DESIGN.md section 10.3.  The bar is test_gpu_dtree.py's and
test_gpu_rforest.py's: every node field, the offsets and the predictions equal the Python
restatement's, under both impurities.  tests/test_tree_shape_cases.py shows off the device that
the restatement alone meets the condition each case exists for."""
import numpy as np
import pytest
import torch

import dtree_reference as D
import rforest_reference as R
import tree_shape_cases as T
import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import classification as clf
from test_gpu_dtree import same_tree
from test_gpu_rforest import same_forest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0, numerics="exact")
    yield c
    c.close()


def ids(cases):
    return [c.name for c in cases]


def check(ctx, c):
    """Both impurities: the device's tree or forest of the case is the restatement's, and so are
    its predictions on the training rows and on probes.  Returns the device's models."""
    X, y = T.inputs(c)
    P = T.probes(X, 5)
    out = []
    for kind in T.KINDS:
        want = T.restated(c, kind)
        if c.trees:
            got = clf.rforest_train(ctx, X, y, impurity=kind, **T.train_args(c))
            same_forest(got, want)
            for Z in (X, P):
                assert np.array_equal(clf.rforest_predict(ctx, Z, *got), R.predict(*want[:2], Z))
        else:
            got = clf.dtree_train(ctx, X, y, impurity=kind, **T.train_args(c))
            same_tree(got, want)
            for Z in (X, P):
                assert np.array_equal(clf.dtree_predict(ctx, Z, got), D.predict(want, Z))
        out.append(got)
    return out


# ---- A: later trips ------------------------------------------------------------------------------
def test_a1_single_tree_past_the_hist_and_route_strides(ctx):
    assert len(check(ctx, T.A1)[0]) >= 7


def test_a2_weighted_single_tree_past_the_strides(ctx):
    assert len(check(ctx, T.A2)[0][0]) >= 7


@pytest.mark.parametrize("c", T.A3, ids=ids(T.A3))
def test_a3_forest_histograms_take_a_second_trip(ctx, c):
    check(ctx, c)


@pytest.mark.parametrize("c", T.PREDICT_TRAIN, ids=ids(T.PREDICT_TRAIN))
def test_a4_predict_past_the_grid_cap(ctx, c):
    Z = T.predict_rows()
    for kind, got in zip(T.KINDS, check(ctx, c)):
        p = clf.rforest_predict(ctx, Z, *got) if c.trees else clf.dtree_predict(ctx, Z, got)
        want = T.restated_predictions(c, kind)
        bad = np.nonzero(p != want)[0]
        assert bad.size == 0, (kind, bad[:4], bad.size)


def test_a5_more_trees_than_grid_y(ctx):
    (nodes, off), _ = check(ctx, T.A5)
    assert len(off) == T.A5.trees + 1 and np.any(np.diff(off)[T.TREES_PER_TRIP:] > 1)


def test_a6_gathered_sample_past_the_grid_cap(ctx):
    c = T.A6
    X, y = T.inputs(c)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    for kind, host in zip(T.KINDS, check(ctx, c)):
        got = clf.dtree_train(ctx, Xd, yd, impurity=kind, **T.train_args(c))
        same_tree(got, T.restated(c, kind))
        assert got.tobytes() == host.tobytes()


# ---- B: exact boundaries -------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.B1, ids=ids(T.B1))
def test_b1_node_sizes_around_the_lds_bound(ctx, c):
    check(ctx, c)


def test_b2_a_launch_that_fills_lds(ctx):
    c = T.B2
    for tree in check(ctx, c):
        assert T.active_per_level(tree, c.max_depth).max() >= 128


@pytest.mark.parametrize("c", T.B3, ids=ids(T.B3))
def test_b3_pair_loop_edges(ctx, c):
    t = c.pair // T.features_per_node(c)
    for nodes, off in check(ctx, c):
        assert nodes[off[t]]["feature"] == T.decisive_feature(c)


# ---- C: decisive lanes, bins and list positions ----------------------------------------------------
@pytest.mark.parametrize("d,f", [(d, f) for d, fs in T.C1_FEATURES.items() for f in fs])
def test_c1_the_chosen_lane_and_bin_decide(ctx, d, f):
    for s in T.C_SPLITS:
        c = T.c1(d, f, s)
        X, _ = T.inputs(c)
        for tree in check(ctx, c):
            assert tree[0]["feature"] == f, s
            assert tree[0]["threshold"] == D.thresholds(X[:, f], 31)[s], s
            assert len(tree) == 3 and np.all(tree["impurity"][1:] == 0.0), s


@pytest.mark.parametrize("d,f", [(d, f) for d, fs in T.C2_FEATURES.items() for f in fs])
def test_c2_every_root_picks_the_feature(ctx, d, f):
    for nodes, off in check(ctx, T.c2(d, f)):
        assert np.all(nodes["feature"][off[:-1]] == f)


def test_c3_the_feature_wins_from_every_list_position(ctx):
    c = T.C3
    lists = T.root_lists(c)
    for nodes, off in check(ctx, c):
        held = [t for t in range(c.trees) if c.f in lists[t]]
        assert np.all(nodes["feature"][off[held]] == c.f)
        assert {lists[t].index(c.f) for t in held} == set(range(7))
