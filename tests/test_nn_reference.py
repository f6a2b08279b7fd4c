"""train_clf=nn without a GPU: the long-double restatement (tests/nn_reference.py) checked against
finite differences and hand-worked updater steps, the config parser and the host-only C entry
against the definition of DESIGN.md section 10.7, Java's Math.round in the statistics, where the
parity cases land in the kernels' tiling, and the float64 noise floor of every parity case."""
import itertools
import math
from ctypes import byref

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd import classification as clf
import nn_cases
import nn_reference as ref

LD = np.longdouble
EPS = np.finfo(LD).eps
ACTIVATIONS = ("sigmoid", "tanh", "relu", "identity", "softplus", "elu", "softmax")
LOSSES = ("xent", "negativeloglikelihood", "mse", "squared_loss")


def small_problem(out_act):
    """5 rows, d = 3, widths (4, 2).  A softmax or sigmoid output keeps p inside (0, 1) for the
    logarithms; any other output activation is shifted there by its bias."""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((5, 3))
    y = np.array([0.0, 1.0, 1.0, 0.0, 1.0])
    p0 = rng.standard_normal(ref.param_count(3, (4, 2))) * 0.3
    return X, y, p0


@pytest.mark.parametrize("hidden,out,loss", [
    (h, o, l) for h, o, l in itertools.product(ACTIVATIONS, ACTIVATIONS, LOSSES)
    # a logarithm needs p in (0, 1): the log losses go with the two outputs that give that
    if l in ("mse", "squared_loss") or o in ("sigmoid", "softmax")])
def test_gradient_equals_central_difference(hidden, out, loss):
    """The restatement's gradient against (L(p + h e_k) - L(p - h e_k)) / 2h of its own loss.
    The truncation error of the step h is measured, not guessed: FD(h) - FD(h/2) is 3/4 of it and
    FD(h/2) carries 1/4 of it.  The rounding error of a difference of two losses, each the result
    of `ops` long-double operations, is at most ops * eps * |L| / step each."""
    X, y, p0 = small_problem(out)
    spec = dict(d=3, widths=(4, 2), activations=(hidden, out), loss=loss)
    _, g = ref.loss_and_gradient(p0, X, y, spec)
    h = EPS ** (LD(1) / 3)  # balances h^2 truncation against eps / h rounding
    ops = 4 * len(X) * p0.size  # multiply-adds of a forward pass, generously, and the loss
    base = abs(ref.loss_of(p0, X, y, spec))
    for k in range(p0.size):
        def fd(step):
            hi, lo = p0.astype(LD), p0.astype(LD)
            hi[k] += step
            lo[k] -= step
            return (ref.loss_of(hi, X, y, spec) - ref.loss_of(lo, X, y, spec)) / (2 * step)
        coarse, fine = fd(h), fd(h / 2)
        bound = abs(coarse - fine) + 2 * ops * EPS * max(base, LD(1)) / (h / 2)
        assert abs(g[k] - fine) <= bound, (k, g[k], fine, bound)


# f(p) = (c0 p0^2 + c1 p1^2) / 2, so g = c * p; lr = 0.1, mu = 0.5, from p = (1, -2)
C = np.array([2.0, 0.5], dtype=LD)
P_START = np.array([1.0, -2.0], dtype=LD)
LR, MU = LD(1) / 10, LD(1) / 2


def run_updater(name, steps=3):
    p, state, seen = P_START.copy(), ref.updater_state(2), []
    for t in range(1, steps + 1):
        p = p - ref.updater_step(name, C * p, state, LR, MU, t)
        seen.append(p.copy())
    return seen


def assert_steps(got, want):
    for g, w in zip(got, want):
        assert np.all(np.abs(g - np.array(w, dtype=LD)) <= 8 * EPS * np.abs(np.array(w, dtype=LD)))


def test_sgd_first_three_steps():
    # p <- p - lr c p = p (1 - lr c): factors 0.8 and 0.95
    f = [LD(8) / 10, LD(95) / 100]
    assert_steps(run_updater("sgd"), [[f[0] ** t, -2 * f[1] ** t] for t in (1, 2, 3)])


def test_nesterovs_first_three_steps():
    want = []
    for c, p in ((LD(2), LD(1)), (LD(1) / 2, LD(-2))):
        v, seq = LD(0), []
        for _ in range(3):
            g = c * p
            v_new = MU * v - LR * g          # v' = mu v - lr g
            p = p - (MU * v - (1 + MU) * v_new)  # u = mu v - (1 + mu) v'
            v = v_new
            seq.append(p)
        want.append(seq)
    # step 1 by hand: v = 0, v' = -0.2, u = 0.3, p = 0.7; and v' = 0.1, u = -0.15, p = -1.85
    assert abs(want[0][0] - LD(7) / 10) <= 4 * EPS and abs(want[1][0] + LD(185) / 100) <= 4 * EPS
    assert_steps(run_updater("nesterovs"), [[want[0][t], want[1][t]] for t in range(3)])


def test_adam_first_three_steps():
    b1, b2, eps = LD(9) / 10, LD(999) / 1000, LD(1) / 10 ** 8
    want = []
    for c, p in ((LD(2), LD(1)), (LD(1) / 2, LD(-2))):
        m = v = LD(0)
        seq = []
        for t in (1, 2, 3):
            g = c * p
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            p = p - LR * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps)
            seq.append(p)
        want.append(seq)
    # step 1 by hand: m = 0.1 g, sqrt(v) = sqrt(0.001) |g|, the bias factors cancel them: u is
    # lr * sign(g) up to eps, so p = 0.9 and -1.9
    assert abs(want[0][0] - LD(9) / 10) <= 1e-7 and abs(want[1][0] + LD(19) / 10) <= 1e-7
    assert_steps(run_updater("adam"), [[want[0][t], want[1][t]] for t in range(3)])


def test_adagrad_first_three_steps():
    want = []
    for c, p in ((LD(2), LD(1)), (LD(1) / 2, LD(-2))):
        h, seq = LD(0), []
        for _ in range(3):
            g = c * p
            h = h + g * g
            p = p - LR * g / (np.sqrt(h) + LD(1) / 10 ** 6)
            seq.append(p)
        want.append(seq)
    # step 1 by hand: h = g^2, u = lr g / (|g| + 1e-6): p = 1 - 0.2 / 2.000001
    assert abs(want[0][0] - (1 - LD(2) / 10 / (2 + LD(1) / 10 ** 6))) <= 4 * EPS
    assert_steps(run_updater("adagrad"), [[want[0][t], want[1][t]] for t in range(3)])


def test_rmsprop_first_three_steps():
    want = []
    for c, p in ((LD(2), LD(1)), (LD(1) / 2, LD(-2))):
        r, seq = LD(0), []
        for _ in range(3):
            g = c * p
            r = LD(95) / 100 * r + LD(5) / 100 * g * g
            p = p - LR * g / np.sqrt(r + LD(1) / 10 ** 8)
            seq.append(p)
        want.append(seq)
    # step 1 by hand: r = 0.05 * 4 = 0.2, u = 0.2 / sqrt(0.2 + 1e-8)
    assert abs(want[0][0] - (1 - LD(2) / 10 / np.sqrt(LD(2) / 10 + LD(1) / 10 ** 8))) <= 4 * EPS
    assert_steps(run_updater("rmsprop"), [[want[0][t], want[1][t]] for t in range(3)])


# ---- the config keys ----------------------------------------------------------------------------
def readme_config():
    """The keys of the reference's README (its train_clf=nn section) at their defaults, but for
    the optimiser (the default, conjugate_gradient, is refused) and two layers."""
    return {
        "config_seed": "12345", "config_num_iterations": "1000", "config_learning_rate": "0.1",
        "config_momentum": "0.5", "config_weight_init": "xavier", "config_updater": "nesterovs",
        "config_optimization_algo": "stochastic_gradient_descent",
        "config_loss_function": "xent", "config_pretrain": "false", "config_backprop": "true",
        "config_layer1_layer_type": "dense", "config_layer1_drop_out": "0.0",
        "config_layer1_activation_function": "relu", "config_layer1_n_out": "16",
        "config_layer2_layer_type": "output", "config_layer2_drop_out": "0.0",
        "config_layer2_activation_function": "sigmoid", "config_layer2_n_out": "2",
    }


def test_config_of_the_readme_keys():
    m = clf.nn_config_from(readme_config(), 48)
    assert m == clf.NnModel(d=48, widths=(16, 2), activations=("relu", "sigmoid"), loss="xent",
                            updater="nesterovs", learning_rate=0.1, momentum=0.5,
                            num_iterations=1000, seed=12345, weight_init="xavier")
    assert m.param_count == 48 * 16 + 16 + 16 * 2 + 2


def test_config_unknown_strings_map_as_the_reference_maps_them():
    c = readme_config()
    c.update(config_layer1_activation_function="swish", config_loss_function="hinge",
             config_updater="adadelta", config_weight_init="he", config_optimization_algo="sgd",
             config_layer2_layer_type="classification")
    del c["config_layer2_drop_out"]  # parseLayer's default branch reads no drop_out ...
    c["config_layer2_x"] = "1"       # ... and the layer count is the number of keys / 4
    m = clf.nn_config_from(c, 48)
    assert (m.activations, m.loss, m.updater, m.weight_init) == (
        ("sigmoid", "sigmoid"), "mse", "nesterovs", "relu")


REFUSALS = [
    ({"config_layer1_layer_type": "auto_encoder"}, "config_layer1_layer_type=auto_encoder"),
    ({"config_layer1_layer_type": "rbm"}, "config_layer1_layer_type=rbm"),
    ({"config_layer1_layer_type": "graves_lstm"}, "config_layer1_layer_type=graves_lstm"),
    ({"config_layer2_layer_type": "dense"}, "config_layer2_layer_type=dense"),
    ({"config_layer1_layer_type": "output"}, "config_layer1_layer_type=output"),
    ({"config_layer1_drop_out": "0.5"}, "config_layer1_drop_out=0.5"),
    ({"config_layer2_drop_out": "0.1"}, "config_layer2_drop_out=0.1"),
    ({"config_optimization_algo": "line_gradient_descent"},
     "config_optimization_algo=line_gradient_descent"),
    ({"config_optimization_algo": "lbfgs"}, "config_optimization_algo=lbfgs"),
    ({"config_optimization_algo": "conjugate_gradient"},
     "config_optimization_algo=conjugate_gradient"),
    ({"config_pretrain": "true"}, "config_pretrain=true"),
    ({"config_backprop": "false"}, "config_backprop=false"),
    ({"config_layer1_n_out": "0"}, "config_layer1_n_out=0"),
    ({"config_layer1_n_out": "65"}, "config_layer1_n_out=65"),
    ({"config_layer2_n_out": "1"}, "config_layer2_n_out=1"),
    ({"config_layer2_n_out": "3"}, "config_layer2_n_out=3"),
    ({"config_layer1_n_out": "many"}, "config_layer1_n_out=many"),
    ({"config_num_iterations": "-1"}, "config_num_iterations=-1"),
]


@pytest.mark.parametrize("change,names", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_config_refusals_name_key_and_value(change, names):
    c = readme_config()
    c.update(change)
    with pytest.raises(fx.EegfxError) as e:
        clf.nn_config_from(c, 48)
    assert names in str(e.value)
    assert e.value.code in (_lib.EEGFX_EINVAL, _lib.EEGFX_ENOTSUP)


@pytest.mark.parametrize("key", sorted(readme_config()))
def test_config_missing_key_is_named(key):
    c = readme_config()
    del c[key]
    with pytest.raises(fx.EegfxError) as e:
        clf.nn_config_from(c, 48)
    # without one of its four keys layer 2 no longer counts: layer 1 is then a dense last layer
    assert key in str(e.value) or "config_layer1_layer_type=dense" in str(e.value)


def test_config_too_many_layers():
    c = readme_config()
    for i in (3, 4, 5):
        for k in clf.NN_LAYER_KEYS:
            c[f"config_layer{i}_{k}"] = c[f"config_layer2_{k}"]
    with pytest.raises(fx.EegfxError, match="5 layers"):
        clf.nn_config_from(c, 48)


# ---- the host-only C entry ----------------------------------------------------------------------
def c_config(widths, acts=None, loss=0, updater=0, n_layers=None):
    c = _lib.NnConfig()
    c.n_layers = len(widths) if n_layers is None else n_layers
    for i, w in enumerate(widths[:4]):
        c.n_out[i] = w
        c.activation[i] = 0 if acts is None else acts[i]
    c.loss, c.updater = loss, updater
    return c


@pytest.mark.parametrize("d,widths", [(48, (16, 2)), (1, (2,)), (1024, (64, 64, 64, 2)),
                                      (5, (1, 2)), (17, (63, 17, 2))])
def test_param_count_equals_the_restatement(d, widths):
    assert fx.lib().eegfx_nn_param_count(d, byref(c_config(widths))) == ref.param_count(d, widths)


@pytest.mark.parametrize("d,cfg,text", [
    (48, c_config((16, 2), n_layers=0), "0 layers"),
    (48, c_config((16, 2), n_layers=5), "5 layers"),
    (48, c_config((0, 2)), "config_layer1_n_out=0"),
    (48, c_config((65, 2)), "config_layer1_n_out=65"),
    (48, c_config((16, 3)), "config_layer2_n_out=3"),
    (48, c_config((2,), acts=(7,)), "config_layer1_activation_function: code 7"),
    (48, c_config((16, 2), loss=4), "config_loss_function: code 4"),
    (48, c_config((16, 2), updater=-1), "config_updater: code -1"),
    (0, c_config((16, 2)), "d=0"),
    (1025, c_config((16, 2)), "d=1025"),
])
def test_param_count_refusals(d, cfg, text):
    assert fx.lib().eegfx_nn_param_count(d, byref(cfg)) == _lib.EEGFX_EINVAL
    assert text in fx.lib().eegfx_last_error().decode()


def test_init_params_shapes_and_scales():
    """Biases are zero; each weight block has the spread its rule names (checked on a block large
    enough for the sample deviation to sit within 10 % of the rule's)."""
    for init, spread in (("xavier", lambda i, o: math.sqrt(2 / (i + o))),
                         ("relu", lambda i, o: math.sqrt(2 / i)),
                         ("sigmoid", lambda i, o: 4 * math.sqrt(6 / (i + o)) / math.sqrt(3)),
                         ("uniform", lambda i, o: 1 / math.sqrt(i) / math.sqrt(3)),
                         ("zero", lambda i, o: 0.0)):
        m = clf.NnModel(d=512, widths=(64, 2), activations=("tanh", "softmax"), weight_init=init)
        p = clf.nn_init_params(m)
        assert p.shape == (m.param_count,)
        (W1, b1), (W2, b2) = ref.unpack(p, 512, (64, 2), np.float64)
        assert not b1.any() and not b2.any()
        assert abs(W1.std() - spread(512, 64)) <= 0.1 * spread(512, 64)
        assert np.array_equal(p, clf.nn_init_params(m))  # the seed decides
    other = clf.NnModel(d=512, widths=(64, 2), activations=("tanh", "softmax"), seed=1)
    assert not np.array_equal(clf.nn_init_params(other), clf.nn_init_params(
        clf.NnModel(d=512, widths=(64, 2), activations=("tanh", "softmax"))))


# ---- ClassificationStatistics.add ----------------------------------------------------------------
# (score, Math.round(score)) from the specification of Java 7+: floor(x + 1/2) as if computed
# exactly, NaN -> 0, out of long range -> the nearest end of it
ROUND_CASES = [
    (0.5, 1), (0.49999999999999994, 0), (-0.5, 0), (-0.50000000000000011, -1), (1.5, 2),
    (1.4999999999999998, 1), (math.nan, 0), (math.inf, 2 ** 63 - 1), (-math.inf, -2 ** 63),
    (1e300, 2 ** 63 - 1),
]


def expected_counts(round_of_score, label):
    """(tp, tn, fp, fn) of one pair."""
    if label == 0:
        return (0, 1, 0, 0) if round_of_score == 0 else (0, 0, 1, 0)
    return (1, 0, 0, 0) if round_of_score == 1 else (0, 0, 0, 1)


def test_java_round_cases():
    for score, want in ROUND_CASES:
        assert clf.java_round(score) == want, score


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_reference_nn_statistics_rounding_cases(label):
    for score, rounded in ROUND_CASES:
        got = clf.reference_nn_statistics([score], [label])
        assert got.as_tuple() == expected_counts(rounded, label), (score, label)
        if math.isfinite(score):
            assert got.MSE == (label - score) * (label - score)
            assert (got.class1sum, got.class2sum) == ((score, 0.0) if label == 0 else (0.0, score))


def test_reference_nn_statistics_accumulates():
    scores = [0.9, 0.2, 0.6, 0.4, 2.0, -1.0]
    labels = [1.0, 0.0, 0.0, 1.0, 1.0, 0.0]
    got = clf.reference_nn_statistics(scores, labels)
    # 0.9/1 tp; 0.2/0 tn; 0.6/0 fp; 0.4/1 fn; 2.0/1 rounds to 2: fn; -1.0/0 rounds to -1: fp
    assert got.as_tuple() == (1, 1, 2, 2)
    assert got.MSE == pytest.approx(0.01 + 0.04 + 0.36 + 0.36 + 1.0 + 1.0)
    assert got.class1sum == pytest.approx(0.2 + 0.6 - 1.0)
    assert got.class2sum == pytest.approx(0.9 + 0.4 + 2.0)
    assert "MSE: " in repr(got) and "Targets: " in repr(got)


def test_the_other_classifiers_repr_is_unchanged():
    text = repr(clf.ClassificationStatistics(1, 2, 3, 4))
    assert text == ("Number of patterns: 10\nTrue positives: 1\nTrue negatives: 2\n"
                    "False positives: 3\nFalse negatives: 4\nAccuracy: 30.0%\n")


# ---- where the parity cases land ------------------------------------------------------------------
def test_cases_land_in_the_tilings_they_are_named_for():
    c = nn_cases.constants()
    for k in ("kNnThreads", "kNnMaxTileRows", "kNnMinStagedRows", "kNnLdsBytes", "kNnGridCap",
              "kNnAccRegs", "kNnPartialDoubles", "kNnStatThreads", "kNnStatUnroll",
              "kNnStatMaxBlocks"):
        assert k in c, k
    staged = {name: nn_cases.plan_tile(cs["d"], cs["widths"])[1]
              for name, cs in nn_cases.CASES.items()}
    last = nn_cases.LAST_STAGED_D
    assert staged["wide_d_1"] and staged[f"wide_d_{last}"]                # first and last staged d
    assert not staged[f"wide_d_{last + 1}"] and not staged["wide_d_1024"]  # ... read through L2
    assert not staged["wide_d_512"]
    assert all(staged[f"d_{d}"] for d in (1, 16, 17, 48, 64, 65, 512, 1024))  # a narrow layer 1
    assert staged["widest_4_layers"]
    # gradient sums in registers only / also in the workgroup's slab
    regs = c["kNnAccRegs"] * c["kNnThreads"]
    count = lambda name: ref.param_count(nn_cases.CASES[name]["d"], nn_cases.CASES[name]["widths"])
    assert count("updater_sgd") <= regs < count("widest_4_layers") and count("d_1024") > regs
    assert count("hidden_tanh") < c["kNnThreads"]  # threads without a parameter
    # rows: below, at and above one tile; the trip cases around one full trip of the capped grid
    rows, _ = nn_cases.plan_tile(5, (3, 2))
    assert rows == c["kNnMaxTileRows"]
    assert {f"n_{n}" for n in (1, rows - 1, rows, rows + 1)} <= set(nn_cases.CASES)
    trip = nn_cases.TRIP_ROWS
    for n in (trip - 1, trip, trip + 1):
        cs = nn_cases.CASES[f"trip_{n}"]
        assert nn_cases.grid(n, cs["d"], cs["widths"]) == c["kNnGridCap"]
    assert (trip + 1 + rows - 1) // rows > c["kNnGridCap"]  # a second trip for one workgroup
    # the tile shrinks below kNnMaxTileRows where the activations of wide layers fill the LDS
    assert nn_cases.plan_tile(48, (64, 64, 64, 2))[0] < c["kNnMaxTileRows"]
    # every tile fits the budget with at least one row, at the largest model too
    assert nn_cases.plan_tile(1024, (64, 64, 64, 2))[0] >= 1


# ---- the noise floor of every parity case ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nn_cases.CASES))
def test_noise_floor_of_the_parity_case(name):
    """A float64 run with the rows summed in reversed order stays within 1e-11 (relative) of the
    long-double parameters: a 100x margin under the GPU bar of 1e-9."""
    cs = nn_cases.CASES[name]
    X, y, p0 = nn_cases.data(name)
    want, want_scores, _ = nn_cases.reference(name)
    got, scores = ref.train(p0, X, y, nn_cases.spec_of(cs), cs["iterations"], dtype=np.float64,
                            reverse=True)
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    srel = float(np.linalg.norm(scores - want_scores) / np.linalg.norm(want_scores))
    print(f"{name}: params {rel:.3e} scores {srel:.3e}")
    assert rel <= 1e-11 and srel <= 1e-11
