"""train_clf=nn on the device against the long-double restatement
(tests/nn_reference.py): parameters and scores within 1e-9 relative, predictions equal away from
0.5; runs bit-identical to each other, from host and from device rows; non-finite rows, refused
labels, the statistics entry, and the train/test flow."""
import math
from ctypes import byref, c_int32

import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib, pipeline
from eeg_dataanalysispackage_amd import classification as clf
from conftest import DOD02, INFO_TRAIN
import nn_cases
import nn_opt_cases
import nn_reference as ref
from test_nn_reference import ROUND_CASES, expected_counts

pytestmark = pytest.mark.gpu
REL = 1e-9
BAD_LABELS_TEXT = "Input validation failed: labels must be 0.0 or 1.0"
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


def model_of(case):
    return clf.NnModel(d=case["d"], widths=case["widths"], activations=case["activations"],
                       loss=case["loss"], updater=case["updater"],
                       learning_rate=case["learning_rate"], momentum=case["momentum"],
                       num_iterations=case["iterations"])


def device(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()  # the cases' arrays are read-only


def close(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return np.linalg.norm(np.asarray(got) - want) <= REL * max(np.linalg.norm(want), 1e-300)


def bits(a):
    if hasattr(a, "is_cuda"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).tobytes()


# ---- parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nn_cases.CASES))
def test_parity_with_the_restatement(ctx, name):
    case = nn_cases.CASES[name]
    X, y, p0 = nn_cases.data(name)
    want, want_scores, want_pred = nn_cases.reference(name)
    m = model_of(case)
    got, scores = clf.nn_train(ctx, X, y, m, p0)
    pred = clf.nn_predict(ctx, X, m, got)
    for what, a, b in (("params", got, want), ("loss", scores, want_scores),
                       ("predictions", pred, want_pred)):
        b = np.asarray(b, dtype=np.longdouble)
        print(f"{name} {what}: {float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)):.3e}")
    assert close(got, want)
    assert close(scores, want_scores)
    assert close(pred, want_pred)
    away = np.abs(np.asarray(want_pred, dtype=np.float64) - 0.5) > 1e-9
    assert np.array_equal(np.rint(pred[away]), np.rint(np.asarray(want_pred, np.float64)[away]))
    if case["last_row_only"]:
        # only the last row has a feature: layer 1's weight moves through that row alone
        assert got[0] != p0[0]


# ---- bits -----------------------------------------------------------------------------------------
BIT_CASES = ["updater_adam", "widest_4_layers", "wide_d_512", f"n_{nn_cases.plan_tile(5, (3, 2))[0] + 1}"]


@pytest.mark.parametrize("name", BIT_CASES)
def test_twice_and_host_against_device(ctx, name):
    case = nn_cases.CASES[name]
    X, y, p0 = nn_cases.data(name)
    m = model_of(case)
    p1, s1 = clf.nn_train(ctx, X, y, m, p0)
    p2, s2 = clf.nn_train(ctx, X, y, m, p0)
    p3, s3 = clf.nn_train(ctx, device(X), device(y), m, p0)
    assert bits(p1) == bits(p2) == bits(p3) and bits(s1) == bits(s2) == bits(s3)
    q1 = clf.nn_predict(ctx, X, m, p1)
    q3 = clf.nn_predict(ctx, device(X), m, p1)
    assert q3.is_cuda and bits(q1) == bits(q3) == bits(clf.nn_predict(ctx, X, m, p1))


def test_no_iterations_returns_params0(ctx):
    case = nn_cases.CASES["updater_sgd"]
    X, y, p0 = nn_cases.data("updater_sgd")
    got, scores = clf.nn_train(ctx, X, y, model_of(case), p0, num_iterations=0)
    assert bits(got) == bits(p0) and scores.shape == (0,)


def off_by_8(a):
    """A copy of `a` that starts 8 bytes past a 16-byte boundary (host array or device tensor)."""
    if hasattr(a, "is_cuda"):
        buf = torch.empty(a.numel() + 3, dtype=a.dtype, device=a.device)
        start = 1 if buf.data_ptr() % 16 == 0 else 0
        out = buf[start:start + a.numel()].view(a.shape)
        out.copy_(a)
        assert out.data_ptr() % 16 == 8
        return out
    buf = np.empty(a.size + 3, dtype=a.dtype)
    start = 1 if buf.ctypes.data % 16 == 0 else 0
    out = buf[start:start + a.size].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 8 and out.flags.c_contiguous
    return out


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_sentinels_and_buffers_8_bytes_off(ctx, mem):
    name = "updater_nesterovs"
    case = nn_cases.CASES[name]
    X, y, p0 = nn_cases.data(name)
    m = model_of(case)
    want, want_scores = clf.nn_train(ctx, X, y, m, p0)
    want_pred = clf.nn_predict(ctx, X, m, want)
    side = (lambda a: off_by_8(device(a))) if mem == DEV else off_by_8
    band = 5
    pbuf = np.full(p0.size + 2 * band + 1, -7.25)
    sbuf = np.full(case["iterations"] + 2 * band + 1, -7.25)
    pout = pbuf[band + 1:band + 1 + p0.size]     # 8 bytes off as well, whatever the base
    sout = sbuf[band + 1:band + 1 + case["iterations"]]
    if pout.ctypes.data % 16 == 0:
        pout = pbuf[band:band + p0.size]
    if sout.ctypes.data % 16 == 0:
        sout = sbuf[band:band + case["iterations"]]
    Xs, ys = side(X), side(y)
    clf.nn_train(ctx, Xs, ys, m, off_by_8(p0), params_out=pout, scores_out=sout)
    assert bits(pout) == bits(want) and bits(sout) == bits(want_scores)
    assert np.count_nonzero(pbuf == -7.25) == pbuf.size - p0.size
    assert np.count_nonzero(sbuf == -7.25) == sbuf.size - case["iterations"]
    n = case["n"]
    if mem == DEV:
        obuf = torch.full((n + 2 * band + 1,), -7.25, dtype=torch.float64, device="cuda")
        at = band + 1 if (obuf.data_ptr() + 8 * (band + 1)) % 16 == 8 else band
        out = obuf[at:at + n]
        assert out.data_ptr() % 16 == 8
    else:
        obuf = np.full(n + 2 * band + 1, -7.25)
        at = band + 1 if (obuf.ctypes.data + 8 * (band + 1)) % 16 == 8 else band
        out = obuf[at:at + n]
    clf.nn_predict(ctx, Xs, m, want, out=out)
    assert bits(out) == bits(want_pred)
    whole = obuf.cpu().numpy() if mem == DEV else obuf
    assert np.count_nonzero(whole == -7.25) == whole.size - n


# ---- rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_non_finite_feature_in_the_last_row(ctx, bad):
    name = "updater_sgd"  # tanh, softmax, negative log likelihood
    case = nn_cases.CASES[name]
    X, y, p0 = nn_cases.data(name)
    Xb = X.copy()
    Xb[-1, 3] = bad
    m = model_of(case)
    got, _ = clf.nn_train(ctx, Xb, y, m, p0)
    want, _ = ref.train(p0, Xb, y, nn_cases.spec_of(case), case["iterations"])
    finite = np.isfinite(np.asarray(want, dtype=np.float64))
    assert not finite.all()
    assert np.array_equal(np.isfinite(got), finite)
    assert close(got[finite], want[finite])
    # under a clean model the other rows' predictions do not see the bad row of their tile
    clean, _, _ = nn_cases.reference(name)
    clean = np.asarray(clean, dtype=np.float64)
    assert bits(clf.nn_predict(ctx, Xb, m, clean)[:-1]) == bits(clf.nn_predict(ctx, X, m, clean)[:-1])


VALIDATE_TRIP = (nn_cases.constants()["kNnValidateThreads"] *
                 nn_cases.constants()["kNnValidateMaxBlocks"])


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_refused_labels(ctx, mem):
    """0.5, NaN and 2.0 in the first row, the last row and the first row of the validation
    kernel's second grid trip: kBadLabels, and params_out keeps what it held.  -0.0 is class 0."""
    n = VALIDATE_TRIP + 1
    m = clf.NnModel(d=1, widths=(1, 2), activations=("tanh", "softmax"),
                    loss="negativeloglikelihood", num_iterations=1)
    p0 = clf.nn_init_params(m)
    X = np.zeros((n, 1))
    y = np.resize([0.0, 1.0, -0.0], n)
    Xs, ys = (device(X), device(y)) if mem == DEV else (X, y)
    clf.nn_train(ctx, Xs, ys, m, p0)  # -0.0 passes
    for row in (0, n - 1, VALIDATE_TRIP):
        for bad in (0.5, math.nan, 2.0):
            keep = float(ys[row])
            ys[row] = bad
            pout, sout = np.full(p0.size, -7.25), np.full(1, -7.25)
            with pytest.raises(fx.EegfxError) as e:
                clf.nn_train(ctx, Xs, ys, m, p0, params_out=pout, scores_out=sout)
            assert e.value.code == _lib.EEGFX_EINVAL and BAD_LABELS_TEXT in str(e.value)
            assert (pout == -7.25).all() and (sout == -7.25).all()
            ys[row] = keep


def no_iterations_bad_label(mem):
    """67 x 5 rows, widths (4, 2), label 40 = 0.5, a plain-SGD model asked for no iterations."""
    name = "cg_tanh_lr10"
    X, y, p0 = nn_opt_cases.data(name)
    y = y.copy()
    y[40] = 0.5
    m = model_of(nn_opt_cases.CASES[name])
    assert m.optimization_algo == "stochastic_gradient_descent" and X.shape == (67, 5)
    return ((device(X), device(y)) if mem == DEV else (X, y)) + (p0, m)


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_no_iterations_still_validates_the_labels(ctx, mem):
    """num_iterations = 0 under SGD: the rows are staged and the labels validated all the same."""
    Xs, ys, p0, m = no_iterations_bad_label(mem)
    pout = np.full(p0.size, -7.25)
    with pytest.raises(fx.EegfxError) as e:
        clf.nn_train(ctx, Xs, ys, m, p0, num_iterations=0, params_out=pout)
    assert e.value.code == _lib.EEGFX_EINVAL and BAD_LABELS_TEXT in str(e.value)
    assert (pout == -7.25).all()
    ys[40] = 1.0
    got, scores = clf.nn_train(ctx, Xs, ys, m, p0, num_iterations=0, params_out=pout)
    assert got is pout and bits(pout) == bits(p0) and scores.shape == (0,)


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_no_iterations_still_validates_the_labels_through_nn_train_opt(ctx, mem):
    """The same through eegfx_nn_train_opt under EEGFX_NN_OPT_SGD: neither search_out nor
    *iterations_run is written."""
    Xs, ys, p0, m = no_iterations_bad_label(mem)
    pout = np.full(p0.size, -7.25)
    search = np.full(3, -7.25).astype(clf.NN_SEARCH_DTYPE)
    keep = search.copy()
    with pytest.raises(fx.EegfxError) as e:
        clf.nn_train_opt(ctx, Xs, ys, m, p0, num_iterations=0, params_out=pout,
                         search_out=search[:0])
    assert e.value.code == _lib.EEGFX_EINVAL and BAD_LABELS_TEXT in str(e.value)
    cfg, o, run = m.struct(0), m.optimizer(), c_int32(-7)
    assert o.algorithm == _lib.NN_OPTIMIZERS["stochastic_gradient_descent"]
    call = lambda: ctx._call(mem, Xs, fx.lib().eegfx_nn_train_opt, ctx.handle, _lib.ptr(Xs),
                             _lib.ptr(ys), 67, 5, byref(cfg), byref(o), _lib.ptr(p0), _lib.ptr(pout),
                             None, _lib.ptr(search), byref(run), mem)
    with pytest.raises(fx.EegfxError) as e:
        call()
    assert e.value.code == _lib.EEGFX_EINVAL and BAD_LABELS_TEXT in str(e.value)
    assert (pout == -7.25).all() and bits(search) == bits(keep) and run.value == -7
    ys[40] = 1.0
    call()
    assert bits(pout) == bits(p0) and bits(search) == bits(keep) and run.value == 0


def test_argument_checks_before_any_device_call(ctx):
    X, y, p0 = nn_cases.data("updater_sgd")
    m = model_of(nn_cases.CASES["updater_sgd"])
    cfg = m.struct()
    out = np.zeros_like(p0)
    call = lambda n, d, c, it=None: fx.lib().eegfx_nn_train(
        ctx.handle, _lib.ptr(X), _lib.ptr(y), n, d, byref(c), _lib.ptr(p0), _lib.ptr(out), None, HOST)
    assert call(0, 48, cfg) == _lib.EEGFX_EINVAL
    assert call(203, 1025, cfg) == _lib.EEGFX_EINVAL
    bad = m.struct()
    bad.n_out[1] = 3
    assert call(203, 48, bad) == _lib.EEGFX_EINVAL
    assert b"config_layer2_n_out=3" in fx.lib().eegfx_last_error()
    bad = m.struct(-1)
    assert call(203, 48, bad) == _lib.EEGFX_EINVAL
    assert b"config_num_iterations=-1" in fx.lib().eegfx_last_error()
    assert not out.any()
    assert call(203, 48, cfg) == _lib.EEGFX_OK  # scores_out may be NULL
    assert bits(out) == bits(clf.nn_train(ctx, X, y, m, p0)[0])


# ---- eegfx_nn_statistics --------------------------------------------------------------------------
def fsum_stats(scores, labels):
    want = clf.reference_nn_statistics(scores, labels)
    s, a = np.asarray(scores, dtype=np.float64), np.asarray(labels, dtype=np.float64)
    r = np.array([clf.java_round(v) for v in a.tolist()])
    return want.as_tuple(), (math.fsum(((a - s) * (a - s)).tolist()),
                             math.fsum(s[r == 0].tolist()), math.fsum(s[r == 1].tolist()))


def assert_stats(got, counts, sums):
    assert got.as_tuple() == counts
    for g, w in zip((got.MSE, got.class1sum, got.class2sum), sums):
        assert abs(g - w) <= REL * abs(w) or g == w


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_statistics_rounding_cases(ctx, mem):
    side = device if mem == DEV else (lambda a: a)
    for label in (0.0, 1.0):
        for score, rounded in ROUND_CASES:
            got = clf.nn_statistics(ctx, side(np.array([score])), side(np.array([label])))
            assert got.as_tuple() == expected_counts(rounded, label), (score, label)
    # the positive ones in one call (sums of one sign: a sum that cancels has no relative bar),
    # and labels that round: 0.4 is class 0, 1.4 class 1, 2.0 no class
    scores = np.array([s for s, _ in ROUND_CASES if 0 < s < 1e10] * 3)
    labels = np.resize([0.0, 1.0, 0.4, 1.4, 2.0, -0.0], scores.size)
    assert_stats(clf.nn_statistics(ctx, side(scores), side(labels)), *fsum_stats(scores, labels))
    assert clf.nn_statistics(ctx, side(np.zeros(0)), side(np.zeros(0))).as_tuple() == (0, 0, 0, 0)


@pytest.mark.parametrize("mem", [HOST, DEV])
def test_statistics_score_in_every_unroll_slot(ctx, mem):
    """One workgroup, kNnStatUnroll rows per thread a grid stride apart: the one score that is a
    miss sits in each slot in turn, and in the last row."""
    c = nn_cases.constants()
    t, u = c["kNnStatThreads"], c["kNnStatUnroll"]
    n = t * u - 3
    side = device if mem == DEV else (lambda a: a)
    rng = np.random.default_rng(5)
    for row in [k * t + 5 for k in range(u)] + [n - 1]:
        labels = rng.integers(0, 2, size=n).astype(np.float64)
        scores = np.clip(labels + 0.2 * rng.standard_normal(n), labels - 0.45, labels + 0.45)
        base, _ = fsum_stats(scores, labels)
        assert base[2] == base[3] == 0
        scores[row] = 1.5 if labels[row] == 1.0 else -0.75  # rounds to 2 / -1: a miss
        counts, sums = fsum_stats(scores, labels)
        assert counts[2] + counts[3] == 1
        assert_stats(clf.nn_statistics(ctx, side(scores), side(labels)), counts, sums)


def test_statistics_second_trip_of_the_capped_grid(ctx):
    c = nn_cases.constants()
    n = c["kNnStatThreads"] * c["kNnStatUnroll"] * c["kNnStatMaxBlocks"] + 1
    labels = torch.zeros(n, dtype=torch.float64, device="cuda")
    scores = torch.full((n,), 0.25, dtype=torch.float64, device="cuda")
    got = clf.nn_statistics(ctx, scores, labels)
    assert got.as_tuple() == (0, n, 0, 0)
    labels[n - 1] = 1.0
    scores[n - 1] = 1.75  # the one false negative lies in the second trip
    got = clf.nn_statistics(ctx, scores, labels)
    assert got.as_tuple() == (0, n - 1, 0, 1)
    assert abs(got.MSE - ((n - 1) * 0.0625 + 0.5625)) <= REL * got.MSE
    assert abs(got.class1sum - (n - 1) * 0.25) <= REL * got.class1sum and got.class2sum == 1.75


# ---- the flow -------------------------------------------------------------------------------------
NN_CONFIG = {
    "config_seed": "12345", "config_num_iterations": "20", "config_learning_rate": "0.1",
    "config_momentum": "0.5", "config_weight_init": "xavier", "config_updater": "nesterovs",
    "config_optimization_algo": "stochastic_gradient_descent",
    "config_loss_function": "negativeloglikelihood", "config_pretrain": "false",
    "config_backprop": "true",
    "config_layer1_layer_type": "dense", "config_layer1_drop_out": "0.0",
    "config_layer1_activation_function": "tanh", "config_layer1_n_out": "16",
    "config_layer2_layer_type": "output", "config_layer2_drop_out": "0.0",
    "config_layer2_activation_function": "softmax", "config_layer2_n_out": "2",
}


@pytest.mark.parametrize("args,epochs", [([INFO_TRAIN], 11), ([DOD02 + ".eeg", "4"], 27)],
                         ids=["infoTrain", "DoD_2015_02"])
def test_run_train_clf(ctx, args, epochs):
    from oracle import oracle
    odp = fx.OffLineDataProvider(args, context=ctx)
    try:
        odp.loadData()
        fe = fx.WaveletTransform(8, 512, 175, 16, context=ctx)
        c = clf.NeuralNetworkClassifier(ctx)
        c.setConfig(NN_CONFIG)
        stats = pipeline.run_train_clf(odp, c, fe)
        data, labels = odp.getData(), odp.getDataLabels()
        assert len(labels) == epochs
        tr, te = pipeline.reference_split(len(labels))
        assert stats.getNumberOfPatterns() == len(te)
        # the host route: train / test on epochs
        h = clf.NeuralNetworkClassifier(ctx)
        h.setConfig(NN_CONFIG)
        h.train(data[tr], [labels[i] for i in tr], fe)
        assert bits(h.params) == bits(c.params) and bits(h.scores) == bits(c.scores)
        host_stats = h.test(data[te], [labels[i] for i in te])
        assert host_stats.as_tuple() == stats.as_tuple()
        for a, b in ((stats.MSE, host_stats.MSE), (stats.class1sum, host_stats.class1sum),
                     (stats.class2sum, host_stats.class2sum)):
            assert abs(a - b) <= REL * abs(b) or a == b
        # the restatement on the oracle's features
        ep, lab, _, err = oracle.data_provider(args)
        assert not err and len(lab) == epochs
        feats = oracle.extract_features(ep)
        m = clf.nn_config_from(NN_CONFIG, 48)
        assert m == c.model
        want, want_scores = ref.train(clf.nn_init_params(m), feats[tr], np.array(lab)[tr],
                                      dict(d=48, widths=m.widths, activations=m.activations,
                                           loss=m.loss, updater=m.updater,
                                           learning_rate=m.learning_rate, momentum=m.momentum),
                                      m.num_iterations)
        assert close(c.params, want) and close(c.scores, want_scores)
        want_stats = clf.reference_nn_statistics(
            ref.predict(want, feats[te], dict(d=48, widths=m.widths, activations=m.activations)),
            np.array(lab)[te])
        assert stats.as_tuple() == want_stats.as_tuple()
    finally:
        odp.close()
