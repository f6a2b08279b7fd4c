"""The train/test flow on the device: the row gather and the confusion
counts of csrc/flow.hip through the C ABI, OffLineDataProvider.split against getFeatures and the
Python restatement of the Java shuffle, and run_train_clf against the host route
(train_test_features, then the module functions on numpy) for the four classifiers.

The gather is compared bit for bit (int64 views) with numpy's src[idx]; the counts with
classification.reference_statistics; a split with getFeatures(...)[perm], which the earlier suites
pin against the oracle and the reference's goldens."""
import os
import re

import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib, classification as clf, pipeline
from eeg_dataanalysispackage_amd._lib import ptr
from conftest import INFO_TRAIN, REPO
from odp_multi_data import alternating, synth, synthetic_directory, write_brainvision

pytestmark = pytest.mark.gpu

GUARD = 64                       # doubles of sentinel on either side of dst
SENT = np.float64(-1.2345e300)
SPECIALS = np.array([0x7FF8000000000123, 0x7FF0000000000001, 0xFFF8DEADBEEF0001,  # NaN payloads
                     0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000],  # +-Inf, -0.0
                    dtype=np.uint64).view(np.int64)
DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST


def launch_constant(name):
    text = open(os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc", "launch.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rows_with_specials(rng, n, d):
    src = rng.standard_normal((n, d))
    flat = src.view(np.int64).reshape(-1)
    at = rng.integers(0, flat.size, size=min(flat.size, 24))
    flat[at] = SPECIALS[np.arange(at.size) % SPECIALS.size]
    return src


def cuda_doubles(count, fill=None):
    """A device buffer of `count` doubles that starts on a 16-byte boundary."""
    buf = torch.empty(count + 1, dtype=torch.float64, device="cuda")
    buf = buf[(buf.data_ptr() % 16) // 8:][:count]
    assert buf.data_ptr() % 16 == 0
    if fill is not None:
        buf.fill_(float(fill))
    return buf


def gather(ctx, src, idx, mem, off_src=0, off_dst=0, d=None, n_src=None):
    """eegfx_gather_rows on one side; src / dst start off_src / off_dst doubles past a 16-byte
    boundary (device).  Returns (status, dst rows); asserts the sentinels around dst."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    n_src = src.shape[0] if n_src is None else n_src
    d = (src.shape[1] if src.ndim == 2 else 1) if d is None else d
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    m = idx.size
    cells = m * max(d, 0)
    lo = GUARD + off_dst
    if mem == DEV:
        s = cuda_doubles(src.size + off_src + 1)[off_src:off_src + src.size]
        s.copy_(torch.from_numpy(src.reshape(-1)))
        i = torch.from_numpy(idx).cuda()
        whole = cuda_doubles(cells + 2 * GUARD + 2, SENT)
        dst = whole[lo:lo + cells]
        assert s.data_ptr() % 16 == 8 * (off_src % 2) and dst.data_ptr() % 16 == 8 * (off_dst % 2)
        torch.cuda.synchronize()
        rc = fx.lib().eegfx_gather_rows(ctx.handle, ptr(s), n_src, d, ptr(i), m, ptr(dst), mem)
        whole = whole.cpu().numpy()
    else:
        whole = np.full(cells + 2 * GUARD + 2, SENT)
        dst = whole[lo:lo + cells]
        rc = fx.lib().eegfx_gather_rows(ctx.handle, ptr(src), n_src, d, ptr(idx), m, ptr(dst), mem)
    assert (whole[:lo] == SENT).all() and (whole[lo + cells:] == SENT).all()
    return rc, whole[lo:lo + cells].reshape(m, max(d, 0))


def index_patterns(rng, n_src, m):
    return {"identity": np.arange(m), "reversed": n_src - 1 - np.arange(m),
            "all-equal": np.full(m, min(7, n_src - 1)), "random": rng.integers(0, n_src, size=m)}


# ---- gather -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 47, 48, 49, 64, 65, 1535, 1536])
def test_gather_equals_numpy_bit_for_bit(ctx, d):
    rng = np.random.default_rng(d)
    src = rows_with_specials(rng, 300, d)
    one = rows_with_specials(rng, 1, d)
    for m in (0, 1, 63, 64, 65, 257):
        for mem in (DEV, HOST):
            for name, idx in index_patterns(rng, 300, m).items():
                rc, out = gather(ctx, src, idx, mem)
                assert rc == _lib.EEGFX_OK, (m, mem, name)
                assert np.array_equal(bits(out), bits(src[idx])), (m, mem, name)
            rc, out = gather(ctx, one, np.zeros(m, dtype=np.int64), mem)  # n_src = 1
            assert rc == _lib.EEGFX_OK and np.array_equal(bits(out), bits(one[np.zeros(m, int)]))


@pytest.mark.parametrize("d", [2, 3, 48, 49, 1535, 1536])
@pytest.mark.parametrize("off_src,off_dst", [(1, 1), (1, 0), (0, 1)])
def test_gather_from_and_to_buffers_8_bytes_off(ctx, d, off_src, off_dst):
    """Even d on a 16-byte boundary takes the 16-byte pieces (the case above); the same d from or
    to a buffer one double off, and every odd d, must take the 8-byte pieces."""
    rng = np.random.default_rng(100 + d)
    src = rows_with_specials(rng, 90, d)
    for m in (1, 65, 257):
        idx = rng.integers(0, 90, size=m)
        rc, out = gather(ctx, src, idx, DEV, off_src, off_dst)
        assert rc == _lib.EEGFX_OK
        assert np.array_equal(bits(out), bits(src[idx])), m


@pytest.mark.parametrize("d", [1, 2, 3])
def test_gather_second_trip_of_the_capped_grid(ctx, d):
    """More pieces than one trip of the capped grid moves: the second trip runs and its last
    unrolled step is partly filled (d = 2: 16-byte pieces, d = 1 and 3: 8-byte pieces)."""
    trip = (launch_constant("kGatherMaxBlocks") * launch_constant("kGatherThreads")
            * launch_constant("kGatherUnroll"))
    dv = 1 if d == 2 else d
    m = (trip + launch_constant("kGatherMaxBlocks") * launch_constant("kGatherThreads") // 2
         + 3 * 64 + 5) // dv + 1
    rng = np.random.default_rng(7)
    src = torch.from_numpy(rows_with_specials(rng, 1000, d)).cuda()
    idx = torch.from_numpy(rng.integers(0, 1000, size=m)).cuda()
    out = pipeline.gather_rows(ctx, src, idx)
    ctx.synchronize()
    assert torch.equal(out.view(torch.int64), src[idx].view(torch.int64))


@pytest.mark.parametrize("n_src,d", [(14_000_000, 48), (1_400_000, 1536)])
def test_gather_past_32_bit_offsets(ctx, n_src, d):
    """Byte offsets past 2^32 (5.4 GB of 48-wide rows) and element offsets past 2^31 (17.2 GB of
    1536-wide rows): the buffer stays uninitialised but for the 130 gathered rows near its end."""
    need = n_src * d * 8
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * need:
        print(f"skipped: {free} bytes free on the device, the case needs 2 x {need}")
        pytest.skip("not enough free device memory")
    rng = np.random.default_rng(n_src % 1000)
    rows = n_src - 1 - 3 * np.arange(130)
    assert (rows[-1] * d * 8 > 2 ** 32) and (d < 1536 or rows[-1] * d > 2 ** 31)
    vals = rows_with_specials(rng, 130, d)
    src = torch.empty((n_src, d), dtype=torch.float64, device="cuda")
    at = torch.from_numpy(rows).cuda()
    for k in range(130):  # plain slices: nothing but these rows is written
        src[int(rows[k])].copy_(torch.from_numpy(vals[k]))
    order = rng.permutation(130)
    out = pipeline.gather_rows(ctx, src, at[torch.from_numpy(order).cuda()])
    ctx.synchronize()
    got = out.cpu().numpy()
    del src, out
    assert np.array_equal(bits(got), bits(vals[order]))


@pytest.mark.parametrize("mem", [DEV, HOST])
@pytest.mark.parametrize("d", [1, 48, 49])
def test_gather_index_out_of_range(ctx, d, mem):
    rng = np.random.default_rng(3)
    src = rows_with_specials(rng, 50, d)
    for bad_value in (-1, 50):
        idx = rng.integers(0, 50, size=130)
        idx[[17, 99]] = bad_value
        rc, out = gather(ctx, src, idx, mem)
        assert rc == _lib.EEGFX_ERANGE
        assert "idx[17]" in fx.lib().eegfx_last_error().decode()
        ok = np.ones(130, dtype=bool)
        ok[[17, 99]] = False
        assert np.array_equal(bits(out[ok]), bits(src[idx[ok]]))
        assert (out[~ok] == SENT).all()  # nothing was copied for those rows
    with pytest.raises(IndexError):
        pipeline.gather_rows(ctx, src, np.array([0, 50]))
    rc, _ = gather(ctx, np.zeros((0, d)), np.array([0]), mem, n_src=0, d=d)  # no row to take
    assert rc == _lib.EEGFX_ERANGE


@pytest.mark.parametrize("mem", [DEV, HOST])
def test_gather_row_width_limits(ctx, mem):
    flat = np.zeros(4 * 1537)
    for d in (0, 1537, -1):
        rc, _ = gather(ctx, flat, np.array([0, 1]), mem, d=d, n_src=4)
        assert rc == _lib.EEGFX_EINVAL, d
    rc, _ = gather(ctx, flat, np.array([], dtype=np.int64), mem, d=16, n_src=4)
    assert rc == _lib.EEGFX_OK  # m == 0


# ---- confusion counts ---------------------------------------------------------------------------
def raw_counts(ctx, pred, labels, mem):
    pred = np.ascontiguousarray(pred, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.float64)
    counts = np.full(4, -9, dtype=np.int64)
    if mem == DEV:
        p, a = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
        torch.cuda.synchronize()
    else:
        p, a = pred, labels
    rc = fx.lib().eegfx_confusion_counts(ctx.handle, ptr(p), ptr(a), pred.size, ptr(counts), mem)
    return rc, tuple(int(v) for v in counts)


def labelled(rng, n, outliers):
    labels = rng.integers(0, 2, size=n).astype(np.float64)
    labels[0], labels[1] = 0.0, 1.0  # both actual classes, whatever the draw
    pred = rng.integers(0, 2, size=n).astype(np.float64)
    if outliers:
        at = rng.integers(0, n, size=max(1, n // 5))
        pred[at] = np.array([np.nan, 0.5, 2.0])[np.arange(at.size) % 3]
    return pred, labels


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 3_000_001])
def test_confusion_counts_equal_reference_statistics(ctx, n):
    rng = np.random.default_rng(n)
    for outliers in (False, True):
        if n > 10 ** 6 and not outliers:
            continue  # the Python reference takes a second per million rows: one pass
        pred, labels = labelled(rng, n, outliers)
        want = clf.reference_statistics(pred, labels).as_tuple()
        if outliers:
            assert sum(want) < n  # NaN, 0.5 and 2.0 fall out of the matrix
        for mem in (DEV, HOST):
            assert raw_counts(ctx, pred, labels, mem) == (_lib.EEGFX_OK, want), mem
    if n <= 10 ** 6:
        pred, labels = labelled(rng, n, False)
        pred[:] = 0.0
        want = clf.reference_statistics(pred, labels).as_tuple()
        assert want[0] == want[3] == 0
        assert raw_counts(ctx, pred, labels, DEV) == (_lib.EEGFX_OK, want)
        got = clf.confusion_counts(ctx, torch.from_numpy(pred).cuda(),
                                   torch.from_numpy(labels).cuda())
        assert got == want == clf.confusion_counts(ctx, pred, labels)


@pytest.mark.parametrize("mem", [DEV, HOST])
def test_confusion_counts_of_one_actual_class(ctx, mem):
    for labels in (np.ones(130), np.zeros(130), np.zeros(0)):
        pred = np.resize([0.0, 1.0], labels.size)
        assert raw_counts(ctx, pred, labels, mem)[0] == _lib.EEGFX_ERANGE
        with pytest.raises(IndexError):
            clf.reference_statistics(pred, labels)
        with pytest.raises(IndexError):
            if mem == DEV:
                clf.confusion_counts(ctx, torch.from_numpy(pred).cuda(),
                                     torch.from_numpy(labels).cuda())
            else:
                clf.confusion_counts(ctx, pred, labels)


@pytest.mark.parametrize("mem", [DEV, HOST])
@pytest.mark.parametrize("bad", [0.5, np.nan, -1.0])
def test_confusion_counts_label_validation(ctx, mem, bad):
    for labels in (np.resize([0.0, 1.0], 131), np.ones(131)):  # checked before the class count
        labels = labels.copy()
        labels[77] = bad
        rc, _ = raw_counts(ctx, np.zeros(131), labels, mem)
        assert rc == _lib.EEGFX_EINVAL
        assert "labels must be 0.0 or 1.0" in fx.lib().eegfx_last_error().decode()


# ---- split --------------------------------------------------------------------------------------
def make_contexts(k):
    n_dev = fx.device_count()
    return [fx.Context(i % n_dev) for i in range(k)]


FE_PARAMS = [(175, 16), (100, 64), (238, 512), (175, 5)]


def check_split(odp, skip, fs, context=None):
    n = odp.num_epochs()
    perm = np.array(pipeline.java_shuffle_permutation(n, 1), dtype=np.int64)
    want_x = odp.getFeatures(8, 512, skip, fs)[perm]
    want_y = np.array(odp.getDataLabels())[perm]
    fe = fx.WaveletTransform(8, 512, skip, fs)
    cut = int(n * 0.7)
    parts = {}
    for device in (True, False):
        xa, ya, xb, yb = odp.split(fe, device=device, context=context)
        if device:
            assert xa.is_cuda and ya.is_cuda and xb.is_cuda and yb.is_cuda
            base = xa.untyped_storage().data_ptr()  # views of one allocation
            assert all(t.untyped_storage().data_ptr() == base for t in (ya, xb, yb))
            xa, ya, xb, yb = (t.cpu().numpy() for t in (xa, ya, xb, yb))
        assert xa.shape == (cut, 3 * fs) and xb.shape == (n - cut, 3 * fs)
        assert ya.shape == (cut,) and yb.shape == (n - cut,)
        parts[device] = (np.concatenate([xa, xb]), np.concatenate([ya, yb]))
        assert np.array_equal(bits(parts[device][0]), bits(want_x)), (skip, fs, device)
        assert np.array_equal(parts[device][1], want_y)
    return parts[True]


@pytest.fixture(scope="module")
def syn_info(tmp_path_factory):
    return synthetic_directory(tmp_path_factory.mktemp("flow_syn"))


@pytest.mark.parametrize("which", ["infoTrain", "synthetic"])
def test_split_is_the_shuffled_getfeatures(which, syn_info):
    args = [INFO_TRAIN if which == "infoTrain" else syn_info]
    per_k = {}
    for k in (1, 3):  # EXACT numerics: three contexts give the one context's bits
        ctxs = make_contexts(k)
        odp = fx.OffLineDataProvider(args, contexts=ctxs)
        odp.loadData()
        assert odp.num_epochs() == (11 if which == "infoTrain" else 35)
        per_k[k] = [check_split(odp, skip, fs) for skip, fs in FE_PARAMS]
        if k == 3:  # rows that land on another context than the first
            check_split(odp, 175, 16, context=ctxs[2])
        odp.close()
        for c in ctxs:
            c.close()
    for (x1, y1), (x3, y3) in zip(per_k[1], per_k[3]):
        assert np.array_equal(bits(x1), bits(x3)) and np.array_equal(y1, y3)
    if which == "infoTrain":
        odp = fx.OffLineDataProvider(args)
        odp.loadData()
        labels = np.array(odp.getDataLabels())
        _, ya, _, yb = odp.split(device=False)
        assert np.array_equal(ya, labels[[0, 7, 9, 2, 5, 10, 6]])
        assert np.array_equal(yb, labels[[3, 1, 8, 4]])
        odp.close()


def test_split_fractions_seeds_and_errors(syn_info):
    odp = fx.OffLineDataProvider([syn_info])
    odp.loadData()
    feats, labels = odp.getFeatures(), np.array(odp.getDataLabels())
    for device in (True, False):
        xa, ya, xb, yb = odp.split(train_fraction=0.0, device=device)
        assert tuple(xa.shape) == (0, 48) and tuple(ya.shape) == (0,)
        assert tuple(xb.shape) == (35, 48)
        xa, ya, xb, yb = odp.split(train_fraction=1.0, device=device)
        assert tuple(xb.shape) == (0, 48) and tuple(yb.shape) == (0,)
        assert tuple(xa.shape) == (35, 48)
    perm = pipeline.java_shuffle_permutation(35, -3)
    xa, ya, xb, yb = odp.split(seed=-3, train_fraction=0.5, device=False)
    assert xa.shape == (17, 48)
    assert np.array_equal(bits(np.concatenate([xa, xb])), bits(feats[perm]))
    assert np.array_equal(np.concatenate([ya, yb]), labels[perm])
    for device in (True, False):
        with pytest.raises(fx.EegfxError) as e:
            odp.split(train_fraction=1.5, device=device)
        assert e.value.code == _lib.EEGFX_EINVAL
        with pytest.raises(fx.EegfxError) as mine:
            odp.split(fx.WaveletTransform(8, 512, 175, 513), device=device)
        with pytest.raises(fx.EegfxError) as theirs:
            odp.getFeatures(8, 512, 175, 513)
        assert mine.value.code == theirs.value.code != _lib.EEGFX_OK
    odp.close()


def test_split_after_a_second_load_covers_the_appended_rows():
    odp = fx.OffLineDataProvider([INFO_TRAIN])
    odp.loadData()
    odp.loadData()  # a one-context provider appends (the balance carries over: 10 more epochs)
    n = odp.num_epochs()
    assert n > 11
    x, y = check_split(odp, 175, 16)
    assert x.shape == (n, 48) and y.shape == (n,)
    check_split(odp, 100, 64)
    odp.close()


def test_split_of_an_empty_provider(tmp_path):
    d = tmp_path / "syn"
    d.mkdir()
    write_brainvision(d, "none", synth(np.random.default_rng(1), 2000, "INT_16"), [])
    info = tmp_path / "info.txt"
    info.write_text("syn/none.eeg 1\n")
    odp = fx.OffLineDataProvider([str(info)])
    odp.loadData()
    assert odp.num_epochs() == 0
    for device in (True, False):
        parts = odp.split(device=device)
        assert [tuple(p.shape) for p in parts] == [(0, 48), (0,), (0, 48), (0,)]
    odp.close()


# ---- the flow -----------------------------------------------------------------------------------
def finite_directory(tmp_path):
    """Three recordings like the synthetic directory's, without the markers at the very end of a
    recording whose all-zero epochs give NaN rows: 36 epochs the four classifiers can train on."""
    d = tmp_path / "fin"
    d.mkdir()
    rng = np.random.default_rng(77)
    for name, nf, fmt, vec in (("a", 9000, "INT_16", False), ("b", 9500, "IEEE_FLOAT_32", False),
                               ("c", 9003, "INT_16", True)):
        marks = alternating(list(range(150, 150 + 12 * 700, 700)))
        write_brainvision(d, name, synth(rng, nf, fmt), marks, fmt, vec)
    info = tmp_path / "fin_info.txt"
    info.write_text("".join(f"fin/{n}.eeg 1\n" for n in "abc"))
    return str(info)


@pytest.fixture(scope="module")
def providers(tmp_path_factory, syn_info):
    ctx = fx.Context(0)
    out = {}
    for name, info in (("synthetic", syn_info),
                       ("finite", finite_directory(tmp_path_factory.mktemp("flow_fin")))):
        odp = fx.OffLineDataProvider([info], context=ctx)
        odp.loadData()
        fe = fx.WaveletTransform(8, 512, 175, 16, context=ctx)
        out[name] = (odp, fe, pipeline.train_test_features(odp, fe))  # the host route's arrays
    yield ctx, out
    for odp, _, _ in out.values():
        odp.close()
    ctx.close()


LR_CONFIG = {"config_num_iterations": "30", "config_step_size": "1.0",
             "config_mini_batch_fraction": "0.5"}


def host_route(kind, ctx, arrays):
    """The existing module functions on the numpy arrays of train_test_features: (model, stats)."""
    xa, ya, xb, yb = arrays
    if kind == "logreg":
        model = clf.sgd_train(ctx, xa, ya, clf.DEFAULT_NUM_ITERATIONS, clf.DEFAULT_STEP_SIZE,
                              clf.DEFAULT_REG_PARAM, clf.DEFAULT_MINI_BATCH_FRACTION)[0]
        pred = clf.predict(ctx, xb, model)
    elif kind == "logreg-minibatch":
        model = clf.sgd_train(ctx, xa, ya, num_iterations=30, step_size=1.0, reg_param=0.0,
                              mini_batch_fraction=0.5, num_partitions=4)[0]
        pred = clf.predict(ctx, xb, model)
    elif kind == "svm":
        model = clf.svm_sgd_train(ctx, xa, ya, clf.DEFAULT_NUM_ITERATIONS, clf.DEFAULT_STEP_SIZE,
                                  clf.DEFAULT_REG_PARAM, clf.DEFAULT_MINI_BATCH_FRACTION)[0]
        pred = clf.svm_predict(ctx, xb, model)
    elif kind == "dt":
        model = clf.dtree_train(ctx, xa, ya)
        pred = clf.dtree_predict(ctx, xb, model)
    else:
        model = clf.rforest_train(ctx, xa, ya, num_partitions=4)
        pred = clf.rforest_predict(ctx, xb, *model)
    return model, clf.reference_statistics(pred, yb).as_tuple()


def classifier_of(kind, ctx):
    c = {"logreg": clf.LogisticRegressionClassifier, "logreg-minibatch":
         clf.LogisticRegressionClassifier, "svm": clf.SVMClassifier,
         "dt": clf.DecisionTreeClassifier, "rf": clf.RandomForestClassifier}[kind](ctx)
    c.num_partitions = 4
    if kind == "logreg-minibatch":
        c.setConfig(LR_CONFIG)
    return c


def model_of(kind, c):
    return (c.nodes, c.tree_offsets) if kind == "rf" else c.nodes if kind == "dt" else c.weights


def same_model(a, b):
    if isinstance(a, tuple):
        return all(same_model(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


KINDS = ["logreg", "logreg-minibatch", "svm", "dt", "rf"]


@pytest.mark.parametrize("kind", KINDS)
def test_run_train_clf_equals_the_host_route(providers, kind):
    """The same kernels on the same rows: the model is the host route's bit for bit, and so are
    the four counters."""
    ctx, data = providers
    odp, fe, arrays = data["finite"]
    assert np.isfinite(arrays[0]).all() and np.isfinite(arrays[2]).all()
    model, stats = host_route(kind, ctx, arrays)
    c = classifier_of(kind, ctx)
    got = pipeline.run_train_clf(odp, c, fe)
    assert same_model(model_of(kind, c), model)
    assert got.as_tuple() == stats and sum(stats) == len(arrays[3])
    assert c.getFeatureExtraction() is fe
    # fe=None is WaveletTransform(8, 512, 175, 16)
    assert pipeline.run_train_clf(odp, classifier_of(kind, ctx)).as_tuple() == stats


@pytest.mark.parametrize("kind", KINDS)
def test_run_train_clf_on_the_synthetic_directory(providers, kind):
    """Two of its 35 epochs lie wholly past the end of their recording: all-zero epochs, NaN rows.
    The linear models carry the NaNs through (the same weights, bit for bit, and the same
    counters on both routes); the trees refuse a non-finite feature on both routes."""
    ctx, data = providers
    odp, fe, arrays = data["synthetic"]
    assert np.isnan(arrays[0]).any() or np.isnan(arrays[2]).any()
    c = classifier_of(kind, ctx)
    if kind in ("dt", "rf") and np.isnan(arrays[0]).any():
        with pytest.raises(fx.EegfxError) as theirs:
            host_route(kind, ctx, arrays)
        with pytest.raises(fx.EegfxError) as mine:
            pipeline.run_train_clf(odp, c, fe)
        assert mine.value.code == theirs.value.code == _lib.EEGFX_EINVAL
        assert str(mine.value) == str(theirs.value)
        return
    model, stats = host_route(kind, ctx, arrays)
    got = pipeline.run_train_clf(odp, c, fe)
    assert same_model(model_of(kind, c), model)
    assert got.as_tuple() == stats


@pytest.mark.parametrize("kind", KINDS)
def test_train_and_test_are_what_they_were(providers, kind):
    """train(epochs, targets, fe) and test(epochs, targets) after the refactor: the module
    functions on the extracted rows, as before it."""
    ctx, data = providers
    odp, fe, arrays = data["finite"]
    epochs, labels = odp.getData(), odp.getDataLabels()
    tr, te = pipeline.reference_split(len(labels))
    c = classifier_of(kind, ctx)
    c.train(epochs[tr], [labels[i] for i in tr], fe)
    model, stats = host_route(kind, ctx, arrays)
    assert same_model(model_of(kind, c), model)
    assert c.test(epochs[te], [labels[i] for i in te]).as_tuple() == stats
    # testFeatures on host rows, and on device rows with host labels
    assert c.testFeatures(arrays[2], arrays[3]).as_tuple() == stats
    assert c.testFeatures(torch.from_numpy(arrays[2]).cuda(), arrays[3]).as_tuple() == stats
