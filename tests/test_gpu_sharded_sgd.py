"""Data-parallel SGD over shards (csrc/sharded.cpp, logreg.hip's lr_fold_kernel and
lr_count_kernel, eegfx_odp_split_sharded).

One shard must give the bits of the one-context entries, which run the same driver with their
context as its one shard (two doors to the code that test_gpu_logreg_shapes.py pins, the second
also with positions), and those entries leave a lone shard's state behind; k shards are held to the long-double
restatement of tests/logreg_reference.py at that file's bars: weights within 1e-9 relative, the
same iteration count, counts exact.  Context i lives on device i % eegfx_device_count(): a box that
shows one GPU runs every case with its contexts sharing that device."""
import ctypes

import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
import logreg_reference as lr
import sharded_sgd_cases as sc
from conftest import INFO_TRAIN
from eeg_dataanalysispackage_amd import _lib, pipeline
from eeg_dataanalysispackage_amd import classification as clf
from odp_multi_data import alternating, synth, synthetic_directory, write_brainvision

pytestmark = pytest.mark.gpu
MAX_K = 5


@pytest.fixture(scope="module")
def ctxs():
    n_dev = fx.device_count()
    cs = [fx.Context(i % n_dev, numerics="exact") for i in range(MAX_K)]
    yield cs
    for c in cs:
        c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def close(a, b):
    return np.linalg.norm(a - b) <= sc.REL * max(np.linalg.norm(b), 1e-300)


def on(ctx, a):
    return torch.tensor(np.ascontiguousarray(a), device=f"cuda:{ctx.device}")


def contiguous_shards(ctxs, X, y, sizes, with_pos=False):
    out, off = [], 0
    for ctx, n in zip(ctxs, sizes):
        sh = (ctx, on(ctx, X[off:off + n]), on(ctx, y[off:off + n]))
        out.append(sh + (on(ctx, np.arange(off, off + n, dtype=np.int64)),) if with_pos else sh)
        off += n
    return out


def train(shards, c, **kw):
    if c.gradient == "hinge":
        return clf.svm_sgd_train_sharded(shards, c.iters, 1.0, 0.01, convergence_tol=c.tol, **kw)
    return clf.sgd_train_sharded(shards, c.iters, 1.0, 0.01, mini_batch_fraction=c.fraction,
                                 convergence_tol=c.tol,
                                 num_partitions=c.parts if c.fraction < 1.0 else None, **kw)


def states(shards, d):
    """The final LrState of every shard that took part."""
    return [clf.shard_state(sh[0], d) for sh in shards if sh[1].shape[0]]


def check_against_restatement(shards, c):
    w, it = train(shards, c, initial_weights=sc.start(c))
    wr, itr, margin = sc.restated(c)
    err = np.linalg.norm(w - wr) / np.linalg.norm(wr)
    print(f"{sc.case_id(c)}: iterations {it} / {itr}  rel {err:.2e}  conv margin {margin:.2e}")
    assert margin > sc.CONDITIONED
    assert it == itr
    assert close(w, wr)
    for s_it, flag, updates, s_w in states(shards, c.d):   # every shard ends on the root's state
        assert (s_it, flag) == (it, 1) and np.array_equal(bits(s_w), bits(w))
    return w, it


# ---- one shard is the existing trainer ----------------------------------------------------------

@pytest.mark.parametrize("n,d", [(300, 48), (2100, 257)])
@pytest.mark.parametrize("kind", ["logistic", "logistic-0.5", "hinge"])
def test_one_shard_equals_the_one_context_entry_bit_for_bit(ctxs, kind, n, d):
    X, y = lr.rows(n, d, 1000 * d + n)
    ctx = ctxs[0]
    Xd, yd = on(ctx, X), on(ctx, y)
    start = lr.initial_weights(d)
    if kind == "hinge":
        want = clf.svm_sgd_train(ctx, Xd, yd, 100, 1.0, 0.01, initial_weights=start)
        got = clf.svm_sgd_train_sharded([(ctx, Xd, yd)], 100, 1.0, 0.01, initial_weights=start)
    else:
        f = 0.5 if kind.endswith("0.5") else 1.0
        want = clf.sgd_train(ctx, Xd, yd, 100, 1.0, 0.01, mini_batch_fraction=f,
                             initial_weights=start, num_partitions=4)
        got = clf.sgd_train_sharded([(ctx, Xd, yd)], 100, 1.0, 0.01, mini_batch_fraction=f,
                                    initial_weights=start, num_partitions=4)
    assert got[1] == want[1] > 0
    assert np.array_equal(bits(got[0]), bits(want[0]))
    assert not np.array_equal(bits(got[0]), bits(start))
    # an empty shard before and behind it changes nothing
    empty = (on(ctxs[1], np.zeros((0, d))), on(ctxs[1], np.zeros(0)))
    if kind != "logistic-0.5":
        again = (clf.svm_sgd_train_sharded if kind == "hinge" else clf.sgd_train_sharded)(
            [(ctxs[1],) + empty, (ctx, Xd, yd), (ctxs[2], on(ctxs[2], np.zeros((0, d))),
                                                 on(ctxs[2], np.zeros(0)))],
            100, 1.0, 0.01, initial_weights=start)
        assert again[1] == want[1] and np.array_equal(bits(again[0]), bits(want[0]))


@pytest.mark.parametrize("kind", ["logistic", "hinge"])
def test_a_one_context_run_leaves_the_state_of_a_lone_shard(ctxs, kind):
    """The one-context entries run the driver with their context as its one shard:
    eegfx_glm_shard_state reads what they leave, and rows staged from the host give the bits of
    rows on the device."""
    n, d = 300, 48
    X, y = lr.rows(n, d, 1000 * d + n)
    ctx = ctxs[0]
    fn = clf.svm_sgd_train if kind == "hinge" else clf.sgd_train
    w, it = fn(ctx, on(ctx, X), on(ctx, y), 100, 1.0, 0.01)
    s_it, flag, updates, s_w = clf.shard_state(ctx, d)
    assert (s_it, flag) == (it, 1) and it > 0 and updates >= 1
    assert np.array_equal(bits(s_w), bits(w)) and np.any(w != 0.0)
    if kind == "logistic":
        clf.sgd_train(ctx, on(ctx, X[::-1]), on(ctx, y[::-1]), 3, 1.0, 0.01)   # another state
        hw, hit = clf.sgd_train(ctx, X, y, 100, 1.0, 0.01)
        assert hit == it and np.array_equal(bits(hw), bits(w))
        s_it, flag, updates, s_w = clf.shard_state(ctx, d)
        assert (s_it, flag) == (it, 1) and updates >= 1 and np.array_equal(bits(s_w), bits(w))


def test_one_shard_with_positions_equals_the_one_context_entry_bit_for_bit(ctxs):
    """The lone shard's path with a position list, which the one-context entry never takes."""
    n, d = 300, 48
    X, y = lr.rows(n, d, 1000 * d + n)
    ctx = ctxs[0]
    Xd, yd = on(ctx, X), on(ctx, y)
    want = clf.sgd_train(ctx, Xd, yd, 100, 1.0, 0.01, mini_batch_fraction=0.5, num_partitions=4)
    got = clf.sgd_train_sharded([(ctx, Xd, yd, on(ctx, np.arange(n, dtype=np.int64)))], 100, 1.0,
                                0.01, mini_batch_fraction=0.5, num_partitions=4)
    assert got[1] == want[1] > 0 and np.array_equal(bits(got[0]), bits(want[0]))
    assert np.any(got[0] != 0.0)


# ---- k shards against the long-double restatement -----------------------------------------------

@pytest.mark.parametrize("c", sc.FULL_CASES + sc.CONVERGING, ids=sc.case_id)
def test_shards_equal_the_restatement(ctxs, c):
    X, y = sc.rows(c)
    _, it = check_against_restatement(contiguous_shards(ctxs, X, y, c.sizes), c)
    if c.tol != 0.001:
        assert it < c.iters - 1     # converged early: the later launches left every state alone


@pytest.mark.parametrize("c", sc.FEW_ITERATIONS, ids=sc.case_id)
def test_zero_and_one_iteration(ctxs, c):
    X, y = sc.rows(c)
    w, it = check_against_restatement(contiguous_shards(ctxs, X, y, c.sizes), c)
    assert it == c.iters
    if c.iters == 0:
        assert np.array_equal(bits(w), bits(sc.start(c)))


@pytest.mark.parametrize("c", sc.SCATTER_CASES, ids=sc.case_id)
def test_mini_batch_over_scattered_positions(ctxs, c):
    X, y = sc.rows(c)
    lists = sc.interleaved(c)
    n = sum(c.sizes)
    assert sorted(np.concatenate(lists).tolist()) == list(range(n))
    assert all(np.all(np.diff(p) > 1) for p in lists)               # interleaved, not contiguous
    assert all(len(set((p // 32).tolist())) > 1 for p in lists)     # more than one mask word
    samples = [set(sc.sample_rows(c)(i)) for i in range(1, c.iters + 1)]
    if c.fraction == 0.03:
        assert any(not s for s in samples)                          # an empty sample
        assert any(s and any(not s & set(p.tolist()) for p in lists) for s in samples)
    shards = [(ctx, on(ctx, X[p]), on(ctx, y[p]), on(ctx, p)) for ctx, p in zip(ctxs, lists)]
    check_against_restatement(shards, c)


@pytest.mark.parametrize("c", sc.CONTIGUOUS_SAMPLED, ids=sc.case_id)
def test_mini_batch_without_positions(ctxs, c):
    """pos == NULL: shard s holds the positions behind shard s - 1's; the same bits as with the
    positions spelled out."""
    X, y = sc.rows(c)
    w, it = check_against_restatement(contiguous_shards(ctxs, X, y, c.sizes), c)
    w2, it2 = train(contiguous_shards(ctxs, X, y, c.sizes, with_pos=True), c,
                    initial_weights=sc.start(c))
    assert it2 == it and np.array_equal(bits(w2), bits(w))


@pytest.mark.parametrize("c", [sc.FULL_CASES[2], sc.FULL_CASES[-1], sc.SCATTER_CASES[1]],
                         ids=sc.case_id)
def test_two_runs_give_the_same_bits(ctxs, c):
    X, y = sc.rows(c)
    if c.fraction < 1.0:
        shards = [(ctx, on(ctx, X[p]), on(ctx, y[p]), on(ctx, p))
                  for ctx, p in zip(ctxs, sc.interleaved(c))]
    else:
        shards = contiguous_shards(ctxs, X, y, c.sizes)
    w1, it1 = train(shards, c)
    s1 = states(shards, c.d)
    w2, it2 = train(shards, c)
    assert it1 == it2 and np.array_equal(bits(w1), bits(w2))
    for (a_it, a_flag, a_up, a_w), (b_it, b_flag, b_up, b_w) in zip(s1, states(shards, c.d)):
        assert (a_it, a_flag, a_up) == (b_it, b_flag, b_up) == (it1, 1, s1[0][2])
        assert np.array_equal(bits(a_w), bits(w1)) and np.array_equal(bits(b_w), bits(w1))


# ---- refusals -----------------------------------------------------------------------------------

def raw_train(grad, shards, d, w, fraction=1.0, iters=100):
    """The entry itself on a caller's weight array: (status, message)."""
    arr, keep, _, _ = clf._glm_shards(shards)
    torch.cuda.synchronize()
    it = ctypes.c_int32(-5)
    rc = fx.lib().eegfx_glm_sgd_train_sharded(grad, arr, len(shards), d, iters, 1.0, 0.01,
                                              fraction, 0.001, 4, _lib.ptr(w), ctypes.byref(it))
    return rc, fx.lib().eegfx_last_error().decode(), it.value


def one_context_error(fn, *args, **kw):
    with pytest.raises(fx.EegfxError) as e:
        fn(*args, **kw)
    return e.value.code, str(e.value).split("] ", 1)[1]


def test_refusals_are_the_one_context_entry_s(ctxs):
    d = 48
    X, y = lr.rows(313, d, 5)
    start = lr.initial_weights(d)
    ctx = ctxs[0]

    def refused(grad, shards, want, **kw):
        w = start.copy()
        rc, msg, it = raw_train(grad, shards, d, w, **kw)
        assert (rc, msg) == want, (rc, msg, want)
        assert np.array_equal(bits(w), bits(start)) and it == -5    # untouched

    # a label of 0.5 on the last shard only
    yb = y.copy()
    yb[-1] = 0.5
    for grad, fn in ((0, clf.sgd_train), (1, clf.svm_sgd_train)):
        refused(grad, contiguous_shards(ctxs, X, yb, (300, 0, 13)),
                one_context_error(fn, ctx, X, yb))
    # hinge with a fraction of 0.5
    want = one_context_error(clf.svm_sgd_train, ctx, X, y, mini_batch_fraction=0.5)
    assert want[0] == _lib.EEGFX_ENOTSUP
    refused(1, contiguous_shards(ctxs, X, y, (300, 0, 13)), want, fraction=0.5)
    # every shard empty
    want = one_context_error(clf.sgd_train, ctx, X[:0], y[:0])
    refused(0, contiguous_shards(ctxs, X, y, (0, 0, 0)), want)
    refused(0, [], want)
    # a repeated context
    twice = [(ctx, on(ctx, X[:100]), on(ctx, y[:100])), (ctx, on(ctx, X[100:]), on(ctx, y[100:]))]
    w = start.copy()
    rc, msg, _ = raw_train(0, twice, d, w)
    assert rc == _lib.EEGFX_EINVAL and "repeats the context" in msg
    assert np.array_equal(bits(w), bits(start))
    # the bounds of the one-context entry
    for kw, fn_kw in (({"iters": -1}, {"num_iterations": -1}),
                      ({"fraction": -0.5}, {"mini_batch_fraction": -0.5}),
                      ({"fraction": 1.5}, {"mini_batch_fraction": 1.5})):
        refused(0, contiguous_shards(ctxs, X, y, (300, 0, 13)),
                one_context_error(clf.sgd_train, ctx, X, y, **fn_kw), **kw)
    # and the contexts are as good as before
    c = sc.FULL_CASES[2]
    check_against_restatement(contiguous_shards(ctxs, *sc.rows(c), c.sizes), c)


@pytest.mark.parametrize("grad", [0, 1])
def test_a_one_context_run_on_a_bad_label_is_refused_and_leaves_the_context_good(ctxs, grad):
    n, d = 300, 48
    X, y = lr.rows(n, d, 1000 * d + n)
    yb = y.copy()
    yb[-1] = 0.5
    ctx = ctxs[0]
    Xd, yd, ybd = on(ctx, X), on(ctx, y), on(ctx, yb)
    start = lr.initial_weights(d)
    torch.cuda.synchronize()

    def raw(labels, w, it):
        head = (ctx.handle, _lib.ptr(Xd), _lib.ptr(labels), n, d, 100, 1.0, 0.01, 1.0, 0.001)
        tail = (_lib.ptr(w), ctypes.byref(it), _lib.MEM_DEVICE)
        rc = (fx.lib().eegfx_svm_sgd_train(*head, *tail) if grad else
              fx.lib().eegfx_logreg_sgd_train_partitioned(*head, 4, *tail))
        return rc, fx.lib().eegfx_last_error().decode()

    w, it = start.copy(), ctypes.c_int32(-5)
    assert raw(ybd, w, it) == (_lib.EEGFX_EINVAL,
                               "Input validation failed: labels must be 0.0 or 1.0")
    assert np.array_equal(bits(w), bits(start)) and it.value == -5      # untouched
    # the context is as good as a fresh one
    fn = clf.svm_sgd_train if grad else clf.sgd_train
    got = fn(ctx, Xd, yd, 100, 1.0, 0.01, initial_weights=start)
    fresh = fx.Context(ctx.device, numerics="exact")
    try:
        want = fn(fresh, Xd, yd, 100, 1.0, 0.01, initial_weights=start)
    finally:
        fresh.close()
    assert got[1] == want[1] > 0 and np.array_equal(bits(got[0]), bits(want[0]))
    assert not np.array_equal(bits(got[0]), bits(start))


# ---- counts -------------------------------------------------------------------------------------

COUNT_SIZES = [(2, 63, 64, 65, 257), (4 * 2048 + 1, 0, 2)]   # one past a full trip of the grid
KINDS = (("logistic", False, clf.predict, 0.5), ("svm", True, clf.svm_predict, 0.0))


def count_inputs(sizes, d):
    n = sum(sizes)
    X, y = lr.rows(n, d, 9000 + d + n)
    w = 2.0 * np.random.default_rng(6000 + d).standard_normal(d)
    y = y.copy()
    y[:2] = 1.0                                          # sizes[0] == 2: a shard of one class
    return X, y, w, sizes[0] + (5 if sizes[1] else 1)    # and a row of the next shard with rows


@pytest.mark.parametrize("d", [48, 200])
@pytest.mark.parametrize("sizes", COUNT_SIZES, ids=lambda s: "n" + "-".join(map(str, s)))
def test_counts_equal_predict_then_confusion_counts(ctxs, sizes, d):
    X, y, w, nan_row = count_inputs(sizes, d)
    assert set(y) == {0.0, 1.0}
    Xp = X.copy()
    Xp[nan_row, d // 2] = np.nan
    ctx = ctxs[0]
    for kind, svm, predict, t in KINDS:
        for rows_, b in ((X, 0.0), (X, 0.25), (Xp, 0.25)):
            shards = contiguous_shards(ctxs, rows_, y, sizes)
            want = clf.confusion_counts(ctx, predict(ctx, rows_, w, b), y)
            got = clf.count_sharded(shards, w, b, threshold=t, svm=svm)
            assert got == want, (kind, b)
            assert sum(got) == sum(sizes)
            host = clf.reference_statistics(predict(ctx, rows_, w, b), y).as_tuple()
            assert got == host
        # clearThreshold: raw scores are predictions of no class and are counted nowhere -- the
        # NaN row's among them
        shards = contiguous_shards(ctxs, Xp, y, sizes)
        raw = predict(ctx, Xp, w, 0.25, threshold=None)
        assert np.isnan(raw[nan_row])
        want = clf.confusion_counts(ctx, raw, y)
        got = clf.count_sharded(shards, w, 0.25, threshold=None, svm=svm)
        assert got == want and sum(got) == int(np.sum((raw == 0.0) | (raw == 1.0)))


def test_count_refusals(ctxs):
    d, sizes = 48, (2, 63, 64)
    X, y, w, _ = count_inputs(sizes, d)
    ones = np.ones_like(y)
    for svm in (False, True):
        with pytest.raises(IndexError) as e:             # one actual class over all shards
            clf.count_sharded(contiguous_shards(ctxs, X, ones, sizes), w, svm=svm)
        assert e.value.code == _lib.EEGFX_ERANGE
        with pytest.raises(IndexError):                  # no rows
            clf.count_sharded(contiguous_shards(ctxs, X, y, (0, 0, 0)), w, svm=svm)
        for yb in (y.copy(), ones.copy()):               # a bad label is reported first
            yb[-1] = 0.5
            with pytest.raises(fx.EegfxError, match="validation") as e:
                clf.count_sharded(contiguous_shards(ctxs, X, yb, sizes), w, svm=svm)
            assert e.value.code == _lib.EEGFX_EINVAL
    twice = [(ctxs[0], on(ctxs[0], X[:9]), on(ctxs[0], y[:9]))] * 2
    with pytest.raises(fx.EegfxError, match="repeats the context"):
        clf.count_sharded(twice, w)


# ---- the split, kept per shard ------------------------------------------------------------------

@pytest.fixture(scope="module")
def syn_info(tmp_path_factory):
    return synthetic_directory(tmp_path_factory.mktemp("sharded_syn"))


def check_split_shards(odp, fe):
    """Every shard's rows scattered by their positions are eegfx_odp_split's X and y, bit for bit."""
    xa, ya, xb, yb = odp.split(fe, device=False)
    split = odp.splitShards(fe)
    assert len(split) == len(odp.getShards())
    for part, X, y in (("train", xa, ya), ("test", xb, yb)):
        gx = np.full(X.shape, np.float64(12345.0))
        gy = np.full(y.shape, np.float64(12345.0))
        filled = np.zeros(len(y), dtype=np.int64)
        for s, shard in zip(split, odp.getShards()):
            sx, sy, sp = (getattr(s, f"{name}_{part}") for name in ("X", "y", "pos"))
            assert s.n_train + s.n_test == shard.count and s.ctx_index == shard.ctx_index
            assert sx.device.index == sy.device.index == sp.device.index == s.context.device
            torch.cuda.synchronize()
            p = sp.cpu().numpy()
            assert np.all(np.diff(p) > 0)
            gx[p], gy[p] = sx.cpu().numpy(), sy.cpu().numpy()
            filled[p] += 1
        assert np.all(filled == 1)
        assert np.array_equal(bits(gx), bits(X)) and np.array_equal(bits(gy), bits(y))
    return split


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("which", ["infoTrain", "synthetic"])
def test_split_shards_scatter_to_the_split(ctxs, syn_info, which, k):
    odp = fx.OffLineDataProvider([INFO_TRAIN if which == "infoTrain" else syn_info],
                                 contexts=ctxs[:k])
    try:
        odp.loadData()
        assert odp.num_epochs() == (11 if which == "infoTrain" else 35)
        check_split_shards(odp, None)                                  # the resident rows
        check_split_shards(odp, fx.WaveletTransform(8, 512, 100, 64))  # rows computed for the call
        odp.loadData()                                                 # a second load starts over
        check_split_shards(odp, None)
        for fraction, n_train in ((0.0, 0), (1.0, odp.num_epochs())):
            split = odp.splitShards(train_fraction=fraction)
            assert sum(s.n_train for s in split) == n_train
            assert all(tuple(s.X_test.shape) == (s.n_test, 48) for s in split)
        with pytest.raises(fx.EegfxError) as e:
            odp.splitShards(train_fraction=1.5)
        assert e.value.code == _lib.EEGFX_EINVAL
    finally:
        odp.close()


def test_split_shards_of_an_appending_and_of_a_planning_provider(ctxs):
    odp = fx.OffLineDataProvider([INFO_TRAIN], context=ctxs[0])
    odp.loadData()
    odp.loadData()          # the one-context provider appends
    assert odp.num_epochs() > 11
    check_split_shards(odp, None)
    odp.close()
    plan = fx.OffLineDataProvider([INFO_TRAIN], plan_only=True, shards=3)
    plan.loadData()
    with pytest.raises(fx.EegfxError) as e:
        plan.splitShards()
    assert e.value.code == _lib.EEGFX_EINVAL
    plan.close()


def test_split_shards_of_an_empty_provider(ctxs, tmp_path):
    d = tmp_path / "syn"
    d.mkdir()
    write_brainvision(d, "none", synth(np.random.default_rng(1), 2000, "INT_16"), [])
    info = tmp_path / "info.txt"
    info.write_text("syn/none.eeg 1\n")
    odp = fx.OffLineDataProvider([str(info)], contexts=ctxs[:3])
    odp.loadData()
    split = odp.splitShards()
    assert [(s.n_train, s.n_test) for s in split] == [(0, 0)] * 3
    assert all(tuple(s.X_train.shape) == (0, 48) for s in split)
    odp.close()


# ---- the flow -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fin_info(tmp_path_factory):
    """A directory like the synthetic one without the markers at the very end of a recording,
    whose all-zero epochs give NaN rows: 36 epochs the linear classifiers train on with finite
    weights (the directory of test_gpu_flow.py's flow tests)."""
    tmp = tmp_path_factory.mktemp("sharded_fin")
    d = tmp / "fin"
    d.mkdir()
    rng = np.random.default_rng(77)
    for name, nf, fmt, vec in (("a", 9000, "INT_16", False), ("b", 9500, "IEEE_FLOAT_32", False),
                               ("c", 9003, "INT_16", True)):
        write_brainvision(d, name, synth(rng, nf, fmt),
                          alternating(list(range(150, 150 + 12 * 700, 700))), fmt, vec)
    info = tmp / "fin_info.txt"
    info.write_text("".join(f"fin/{n}.eeg 1\n" for n in "abc"))
    return str(info)


NEAR = 1e-9


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", ["logreg", "svm"])
@pytest.mark.parametrize("data", ["finite", "synthetic"])
def test_run_train_clf_sharded(ctxs, fin_info, syn_info, data, kind, k):
    cls = clf.LogisticRegressionClassifier if kind == "logreg" else clf.SVMClassifier
    odp = fx.OffLineDataProvider([fin_info if data == "finite" else syn_info], contexts=ctxs[:k])
    try:
        odp.loadData()
        whole, sharded = cls(ctxs[0]), cls()
        want = pipeline.run_train_clf(odp, whole)
        got = pipeline.run_train_clf(odp, sharded, sharded=True)
        w, wr = sharded.weights, whole.weights
        assert sharded.iterations_run == whole.iterations_run
        fin = lr.classes(wr) == 0
        assert np.array_equal(lr.classes(w), lr.classes(wr))
        if data == "finite" or kind == "svm":       # hinge skips a NaN row; logistic carries it
            assert fin.all()
        assert close(w[fin], wr[fin])
        # the statistics: a host recount from the sharded weights, and the unsharded route's
        xa, ya, xb, yb = odp.split(device=False)
        restate = lr.svm_predict if kind == "svm" else lr.predict
        if fin.all():
            clean = np.isfinite(xb).all(axis=1)
            score = np.asarray(restate(xb[clean], w, threshold=None), dtype=np.float64)
            assert np.all(np.abs(score - (0.0 if kind == "svm" else 0.5)) > NEAR)
        with np.errstate(invalid="ignore"):
            pred = np.asarray(restate(xb, w), dtype=np.float64)
        assert got.as_tuple() == clf.reference_statistics(pred, yb).as_tuple()
        assert got.as_tuple() == want.as_tuple()
        assert got.getNumberOfPatterns() == len(yb)
    finally:
        odp.close()


@pytest.mark.parametrize("cls", [clf.DecisionTreeClassifier, clf.RandomForestClassifier,
                                 clf.NeuralNetworkClassifier])
def test_sharded_flow_of_the_other_classifiers_is_not_implemented(ctxs, cls):
    odp = fx.OffLineDataProvider([INFO_TRAIN], contexts=ctxs[:2])
    try:
        odp.loadData()
        with pytest.raises(NotImplementedError, match=cls.__name__):
            pipeline.run_train_clf(odp, cls(ctxs[0]), sharded=True)
    finally:
        odp.close()
