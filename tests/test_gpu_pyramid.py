"""Feature sizes 17..512 on the device (pyramid.hip): a channel's features are the first
feature_size coefficients of the in-place pyramid [a6(8) d6(8) d5(16) d4(32) d3(64) d2(128)
d1(256)] of its 512-sample window (WaveletTransform.java:126-137, :205-212).

Bar: every row equals the oracle's (faithful=True) value for value -- np.array_equal with
NaN == NaN, which also treats -0.0 and 0.0 alike (dwt8.h: the sign of an exactly-zero sum may
differ) -- on every route: device epochs, host epochs (small batches, the 8192-epoch chunks, a
mailbox-enabled context), the raw-recording entry (eegfx_process_recording_fe), and the
provider / WaveletTransform classes; under both numerics settings (wide rows
are EXACT in both, outside the fma guard's counters).  test_oracle_pyramid.py pins the oracle.

Shapes: a sub-tile is 8 signals, so n in {1, 8, 9, 17} with C in {1, 3, 5} gives full, ragged
and several-workgroup launches; the feature sizes sit on both sides of every band edge.
"""
import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
import extreme_inputs as xi
from conftest import INFO_TRAIN
from eeg_dataanalysispackage_amd._lib import check, ptr
from oracle import oracle

pytestmark = pytest.mark.gpu

NFS = (17, 24, 32, 33, 64, 65, 128, 255, 256, 257, 511, 512)
NS, CS, SKIPS = (1, 8, 9, 17), (1, 3, 5), (0, 175, 238)
# three shapes per feature size, walking n, C and skip at different strides, plus the corners
GRID = sorted({(NS[(i + k) % 4], CS[(i + 2 * k) % 3], nf, SKIPS[(i + k) % 3])
               for i, nf in enumerate(NFS) for k in range(3)}
              | {(17, 5, 512, 238), (1, 1, 17, 0), (9, 3, 512, 175), (8, 5, 257, 0)})


@pytest.fixture(scope="module")
def ctx():
    c = fx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_fma():
    c = fx.Context(0, numerics="fma")
    yield c
    c.close()


@pytest.fixture(scope="module")
def epochs():
    """17 x 5 random-normal epochs (x 30); the cases take leading slices.  Read-only."""
    ep = 30.0 * np.random.default_rng(512).standard_normal((17, 5, 750))
    ep.setflags(write=False)
    return ep


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- device epochs ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,nf,sk", GRID)
def test_device_epochs(ctx, epochs, n, C, nf, sk):
    ep = np.ascontiguousarray(epochs[:n, :C])
    want = oracle.extract_features(ep, nfeat=nf, skip=sk)
    got = ctx.extract_features(dev(ep), feature_size=nf, skip=sk).cpu().numpy()
    assert got.shape == (n, C * nf)
    assert eq(got, want)


def test_device_epochs_widest_row(ctx):
    """C = 64, nf = 512: rows of 256 KB."""
    ep = 30.0 * np.random.default_rng(64).standard_normal((9, 64, 750))
    want = oracle.extract_features(ep, nfeat=512)
    assert eq(ctx.extract_features(dev(ep), feature_size=512).cpu().numpy(), want)


# ---- host epochs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("nf", [17, 64, 512])
def test_host_small_batches(ctx, epochs, n, nf):
    """Batches the per-epoch kernel would take at nf <= 16: wide ones must go round it."""
    ep = np.ascontiguousarray(epochs[:n, :3])
    assert eq(ctx.extract_features(ep, feature_size=nf), oracle.extract_features(ep, nfeat=nf))


def test_host_batch_across_the_chunk(ctx):
    ep = 30.0 * np.random.default_rng(8193).standard_normal((8193, 1, 750))
    want = oracle.extract_features(ep, nfeat=33)
    assert eq(ctx.extract_features(ep, feature_size=33), want)


def test_host_wide_call_on_a_mailbox_context(epochs):
    c = fx.Context(0)
    try:
        c.set_mailbox(True)
        ep = np.ascontiguousarray(epochs[:1, :3])
        assert eq(c.extract_features(ep, feature_size=64), oracle.extract_features(ep, nfeat=64))
        ep2 = np.ascontiguousarray(epochs[1:2, :3])
        assert eq(c.extract_features(ep2), oracle.extract_features(ep2))
        assert c.mailbox_state()[0] is True
    finally:
        c.set_mailbox(False)
        c.close()


# ---- the raw-recording entry ---------------------------------------------------------------------
N_FRAMES = 4000
LAYOUTS = {
    "int16_3": (np.int16, 3, [0, 1, 2], [0.1, 0.1, 0.1]),
    "int16_5": (np.int16, 5, [4, 0, 2], [0.1, 0.5, 0.0488281]),
    "int16_32": (np.int16, 32, [31, 0, 7, 16, 3], [0.1, 0.5, 1.0, 0.0488281, 2.5]),
    "float32_4": (np.float32, 4, [3, 1], [1.0, 0.5]),
}
FUSED = [(1, 17, 0), (9, 17, 175), (1, 100, 175), (9, 100, 0), (1, 512, 0), (9, 512, 175)]


def recording(dtype, ct, n_frames=N_FRAMES):
    rng = np.random.default_rng(ct)
    if dtype == np.int16:
        return np.clip(np.rint(-2000 + 600.0 * rng.standard_normal((n_frames, ct))), -32768,
                       32767).astype(np.int16)
    return (50.0 * rng.standard_normal((n_frames, ct))).astype(np.float32)


def positions(n, n_frames=N_FRAMES):
    """Dense overlapping cuts 31 frames apart from the first legal position (both window
    alignments); the last epoch's 750 samples run 450 past the end of the recording."""
    pos = 100 + 31 * np.arange(n, dtype=np.int64)
    pos[-1] = n_frames - 300
    return pos


@pytest.mark.parametrize("n,nf,sk", FUSED)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fused_entry(ctx, layout, n, nf, sk):
    dtype, ct, cols, res = LAYOUTS[layout]
    raw, pos = recording(dtype, ct), positions(n)
    want = oracle.process_recording(raw, cols, res, pos, skip=sk, nfeat=nf)
    got = ctx.process_recording(raw, ct, cols, res, pos, skip=sk, feature_size=nf)
    assert got.shape == (n, len(cols) * nf)
    assert eq(got, want)
    got_d = ctx.process_recording(dev(raw), ct, cols, res, dev(pos), skip=sk, feature_size=nf)
    ctx.synchronize()
    assert eq(got_d.cpu().numpy(), want)
    two = ctx.extract_features(ctx.cut_epochs(raw, ct, cols, res, pos), skip=sk, feature_size=nf)
    assert eq(two, want)


def test_fused_entry_defaults_are_process_recording(ctx):
    dtype, ct, cols, res = LAYOUTS["int16_3"]
    raw, pos = recording(dtype, ct), positions(9)
    out = np.empty((9, 48))
    cols_a, res_a = np.array(cols, np.int32), np.array(res, np.float32)
    check(fx.lib().eegfx_process_recording_fe(
        ctx.handle, ptr(raw), 0, N_FRAMES, ct, ptr(cols_a), ptr(res_a), 3, ptr(pos), 9, 8, 512,
        175, 16, ptr(out), 0))
    assert out.tobytes() == ctx.process_recording(raw, ct, cols, res, pos).tobytes()
    assert eq(out, oracle.process_recording(raw, cols, res, pos))


@pytest.mark.parametrize("nf,sk", [(8, 0), (16, 100)])
def test_fused_entry_narrow_rows_with_another_skip(ctx, nf, sk):
    dtype, ct, cols, res = LAYOUTS["int16_5"]
    raw, pos = recording(dtype, ct), positions(9)
    want = oracle.process_recording(raw, cols, res, pos, skip=sk, nfeat=nf)
    assert eq(ctx.process_recording(raw, ct, cols, res, pos, skip=sk, feature_size=nf), want)


def test_fused_entry_refused_positions(ctx):
    dtype, ct, cols, res = LAYOUTS["int16_3"]
    raw, pos = recording(dtype, ct), positions(9)
    bad = pos.copy()
    bad[4] = 50
    with pytest.raises(fx.EegfxError) as e:
        ctx.process_recording(raw, ct, cols, res, bad, feature_size=64)
    assert e.value.code == -6
    out = ctx.process_recording(dev(raw), ct, cols, res, dev(bad), feature_size=64)
    with pytest.raises(IndexError) as e:
        ctx.synchronize()
    assert e.value.code == -6
    ctx.synchronize()  # the flag was cleared
    keep = np.arange(9) != 4
    want = oracle.process_recording(raw, cols, res, pos[keep], nfeat=64)
    assert eq(out.cpu().numpy()[keep], want)


def test_fused_entry_layout_the_fused_kernels_refuse(ctx):
    """70 int16 channels in the file: one epoch's staged window exceeds a workgroup's LDS
    (wide_supported refuses it); the entry still returns the oracle's rows."""
    cols, res = [69, 0, 35], [0.1, 0.5, 1.0]
    raw, pos = recording(np.int16, 70), positions(9)
    want = oracle.process_recording(raw, cols, res, pos, nfeat=100)
    assert eq(ctx.process_recording(raw, 70, cols, res, pos, feature_size=100), want)
    got = ctx.process_recording(dev(raw), 70, cols, res, dev(pos), feature_size=100)
    ctx.synchronize()
    assert eq(got.cpu().numpy(), want)


# ---- numerics -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [17, 512])
def test_fma_context_returns_the_exact_bytes(ctx, ctx_fma, epochs, nf):
    before = ctx_fma.guard_stats()
    ep = np.ascontiguousarray(epochs[:9, :3])
    a = ctx.extract_features(dev(ep), feature_size=nf).cpu().numpy()
    b = ctx_fma.extract_features(dev(ep), feature_size=nf).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert ctx.extract_features(ep, feature_size=nf).tobytes() == \
        ctx_fma.extract_features(ep, feature_size=nf).tobytes()
    dtype, ct, cols, res = LAYOUTS["int16_5"]
    raw, pos = recording(dtype, ct), positions(9)
    assert ctx.process_recording(raw, ct, cols, res, pos, feature_size=nf).tobytes() == \
        ctx_fma.process_recording(raw, ct, cols, res, pos, feature_size=nf).tobytes()
    assert ctx_fma.guard_stats() == before


# ---- non-finite samples -------------------------------------------------------------------------
@pytest.mark.parametrize("slot", xi.SLOTS)
def test_nan_and_inf_poison_one_row_only(ctx, slot):
    rec, pos = xi.float_recording(), xi.positions(xi.N_A)
    bad = xi.poison(rec, pos[slot], "nan", "window")
    lo, hi = xi.place_range(int(pos[slot]), "window")
    bad[hi - 7, xi.COLS5[2]] = np.inf
    clean = ctx.process_recording(rec, 7, xi.COLS5, xi.RES5, pos, feature_size=512)
    got = ctx.process_recording(bad, 7, xi.COLS5, xi.RES5, pos, feature_size=512)
    assert eq(got, oracle.process_recording(bad, xi.COLS5, xi.RES5, pos, nfeat=512))
    assert np.all(np.isnan(got[slot]))
    keep = np.arange(xi.N_A) != slot
    assert got[keep].tobytes() == clean[keep].tobytes()
    two = ctx.extract_features(ctx.cut_epochs(bad, 7, xi.COLS5, xi.RES5, pos), feature_size=512)
    assert np.all(np.isnan(two[slot])) and two[keep].tobytes() == clean[keep].tobytes()


# ---- provider and classes -----------------------------------------------------------------------
def test_provider_and_wavelet_transform(ctx):
    odp = fx.OffLineDataProvider([INFO_TRAIN], context=ctx)
    odp.loadData()
    ep = odp.getData()
    assert eq(odp.getFeatures(feature_size=64), oracle.extract_features(ep, nfeat=64))
    wt = fx.WaveletTransform(8, 512, 175, 32, context=ctx)
    assert wt.getFeatureDimension() == 96
    want = oracle.extract_features(ep, nfeat=32)
    for i in (0, len(ep) - 1):
        assert eq(wt.extractFeatures(ep[i]), want[i])
    assert eq(wt.extractFeaturesBatch(ep), want)


# ---- limits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,code", [({"feature_size": 513}, -7), ({"epoch_size": 256}, -7),
                                     ({"skip": 239}, -6), ({"feature_size": 0}, -1)])
def test_limits(ctx, epochs, kw, code):
    ep = np.ascontiguousarray(epochs[:2, :3])
    with pytest.raises(fx.EegfxError) as e:
        ctx.extract_features(ep, **kw)
    assert e.value.code == code
    if "epoch_size" not in kw:
        dtype, ct, cols, res = LAYOUTS["int16_3"]
        with pytest.raises(fx.EegfxError) as e:
            ctx.process_recording(recording(dtype, ct), ct, cols, res, positions(2), **kw)
        assert e.value.code == code


# ---- determinism --------------------------------------------------------------------------------
def test_two_launches_give_the_same_bytes(ctx):
    dtype, ct, cols, res = LAYOUTS["int16_32"]
    raw, pos = dev(recording(dtype, ct)), dev(positions(9))
    a = ctx.process_recording(raw, ct, cols, res, pos, feature_size=512)
    b = ctx.process_recording(raw, ct, cols, res, pos, feature_size=512)
    ctx.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
