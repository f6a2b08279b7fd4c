"""Non-finite, subnormal and extreme-magnitude inputs through every epoch-to-feature entry point
and kernel family.  (The classifier entry points -- eegfx_logreg_* / eegfx_svm_* on NaN and +-Inf
feature rows and labels -- are in test_gpu_logreg_shapes.py, their oracle pinned by
test_logreg_reference.py.)

The judge is the CPU oracle, pinned on these very inputs by test_oracle_extremes.py.  One rule
(check) everywhere:

  EXACT  the NaN positions of the oracle's result, and every other value bit-equal (uint64 views:
         the sign of zero and +-Inf count);
  FMA    the same NaN positions and the same +-Inf entries, finite entries within 1e-9.  Epochs
         (cut_epochs, the one-pass epochs) are decoded in the reference's order under both
         numerics, so they are held to the EXACT rule under both.

and one isolation rule wherever an epoch is poisoned: every other epoch's row (or epoch) is
bit-equal to the same call on the clean input, each numerics compared with itself.

A  float32 recordings with a NaN / +Inf / +-Inf pair / -0.0 stretch in one epoch's baseline, window,
   rest, or just past it; the epoch in the full sub-tile and in the ragged last one;
B  float32 magnitudes: subnormal products, products near FLT_MAX, overflowing products;
C  int16 recordings with subnormal, zero, negative, huge and overflowing resolutions, also on the
   window kernels' tracking variants (a launch after one that flagged > 1/16 of its rows);
D  double epochs scaled by 2^k (EXACT invariant; the oracle alone judges 2^505 and 2^-530), with
   NaN / Inf / all-zero epochs among clean ones; device batch and the per-epoch host call with
   the mailbox off and on;
E  a clean launch after every poisoned one on the same context, and the guard's counters.
"""
import functools

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
import extreme_inputs as xi
from oracle import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-9
NUMERICS = ["exact", "fma"]


@pytest.fixture(scope="module")
def ctxs():
    c = {m: fx.Context(0, numerics=m) for m in NUMERICS}
    yield c
    for v in c.values():
        v.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def check(ctx, got, want, what, exact=None):
    """The comparison rule; prints the guard's counters when it fails."""
    got = host(got)
    exact = ctx.numerics == "exact" if exact is None else exact
    try:
        assert got.shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), "NaN positions"
        if exact:
            diff = bits(got)[~nan] != bits(want)[~nan]
            assert not diff.any(), f"{int(diff.sum())} values differ in their bits"
        else:
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(got), inf), "Inf positions"
            assert np.array_equal(got[inf], want[inf]), "Inf signs"
            fin = ~nan & ~inf
            err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
            assert err <= TOL, f"finite entries off by {err}"
    except AssertionError:
        print(f"{what} [{ctx.numerics}]: guard_detail (checked, rechecked, recomputed) = "
              f"{ctx.guard_detail()}")
        raise


def isolated(ctx, got, clean, skip, what):
    """The isolation rule: all epochs but `skip` bit-equal to the clean call's."""
    got, clean = host(got), host(clean)
    keep = [e for e in range(len(got)) if e not in skip]
    if not np.array_equal(bits(got[keep]), bits(clean[keep])):
        bad = [e for e in keep if not np.array_equal(bits(got[e]), bits(clean[e]))]
        print(f"{what} [{ctx.numerics}]: guard_detail = {ctx.guard_detail()}")
        raise AssertionError(f"{what}: epochs {bad} changed with the poison in {sorted(skip)}")


def counters_sane(ctx):
    checked, rechecked, redone = ctx.guard_detail()
    assert 0 <= redone <= rechecked <= checked, (checked, rechecked, redone)
    if ctx.numerics == "exact":
        assert (rechecked, redone) == (0, 0)


# ---- the float32 paths (A, B) --------------------------------------------------------------------
def write_brainvision(tmp_path, name, rec3, pos, res):
    """A float32 .eeg / .vhdr / .vmrk triple whose markers alternate target / non-target, so the
    balanced selection (guessed number 1) keeps every one."""
    rec3.astype("<f4").tofile(str(tmp_path / (name + ".eeg")))
    chans = "".join(f"Ch{i + 1}={nm},,{r},µV\n" for i, (nm, r) in enumerate(zip(("Fz", "Cz", "Pz"), res)))
    (tmp_path / (name + ".vhdr")).write_text(
        "Brain Vision Data Exchange Header File Version 1.0\n\n[Common Infos]\nCodepage=UTF-8\n"
        f"DataFile={name}.eeg\nMarkerFile={name}.vmrk\nDataFormat=BINARY\n"
        "DataOrientation=MULTIPLEXED\nNumberOfChannels=3\nSamplingInterval=1000\n\n"
        "[Binary Infos]\nBinaryFormat=IEEE_FLOAT_32\n\n[Channel Infos]\n" + chans, encoding="utf-8")
    marks = "".join(f"Mk{i + 2}=Stimulus,S  {1 + i % 2},{int(p)},1,0\n" for i, p in enumerate(pos))
    (tmp_path / (name + ".vmrk")).write_text(
        "Brain Vision Data Exchange Marker File, Version 1.0\n\n[Common Infos]\nCodepage=UTF-8\n"
        f"DataFile={name}.eeg\n\n[Marker Infos]\nMk1=New Segment,,1,1,0,20150128095308551177\n"
        + marks, encoding="utf-8")
    return str(tmp_path / (name + ".eeg"))


def float_paths(ctx, rec7, pos, tmp_path=None, tag="rec"):
    """Every path that takes a float32 recording -> {name: (result, 'rows3' | 'rows5' | 'epochs')}."""
    import torch
    rec3 = np.ascontiguousarray(rec7[:, :3])
    out = {}
    out["cut_host"] = (ctx.cut_epochs(rec3, 3, xi.COLS3, xi.RES3, pos), "epochs")
    dev = ctx.cut_epochs(torch.from_numpy(rec3).cuda(), 3, xi.COLS3, xi.RES3,
                         torch.from_numpy(pos).cuda())
    ctx.synchronize()
    out["cut_device"] = (dev.cpu().numpy(), "epochs")
    out["fused_ct3"] = (ctx.process_recording(rec3, 3, xi.COLS3, xi.RES3, pos), "rows3")
    out["fused_ct7"] = (ctx.process_recording(rec7, 7, xi.COLS5, xi.RES5, pos), "rows5")
    f1, e1 = ctx.process_recording_epochs(rec3, 3, xi.COLS3, xi.RES3, pos)
    out["one_pass_rows"], out["one_pass_epochs"] = (f1, "rows3"), (e1, "epochs")
    for chunk in (787, 4099):
        out[f"streamed_{chunk}"] = (ctx.process_recording_streamed(
            rec3, 3, xi.COLS3, xi.RES3, pos, chunk_frames=chunk), "rows3")
    if tmp_path is not None:
        odp = fx.OffLineDataProvider([write_brainvision(tmp_path, tag, rec3, pos, xi.RES3), "1"],
                                     context=ctx)
        try:
            odp.loadData()
            assert odp.last_error == ""
            assert odp.getPositions()[0].tolist() == pos.tolist()
            out["provider_epochs"] = (odp.getData(), "epochs")
            out["provider_rows"] = (odp.getFeatures(), "rows3")
        finally:
            odp.close()
    return out


def float_wants(rec7, pos):
    rec3 = np.ascontiguousarray(rec7[:, :3])
    return {"epochs": oracle.decode_epochs(rec3, xi.COLS3, xi.RES3, pos),
            "rows3": oracle.process_recording(rec3, xi.COLS3, xi.RES3, pos),
            "rows5": oracle.process_recording(rec7, xi.COLS5, xi.RES5, pos)}


@functools.lru_cache(maxsize=None)
def poisoned_want(kind, place, slot):
    pos = xi.positions(xi.N_A)
    return float_wants(xi.poison(xi.float_recording(), pos[slot], kind, place), pos)


@functools.lru_cache(maxsize=None)
def clean_want():
    return float_wants(xi.float_recording(), xi.positions(xi.N_A))


@pytest.fixture(scope="module")
def clean_float(ctxs, tmp_path_factory):
    """The clean float32 recording through every path, per numerics (checked against the oracle)."""
    rec7, pos = xi.float_recording(), xi.positions(xi.N_A)
    want = clean_want()
    res = {}
    for m, ctx in ctxs.items():
        res[m] = float_paths(ctx, rec7, pos, tmp_path_factory.mktemp("clean_" + m))
        for name, (got, kind) in res[m].items():
            check(ctx, got, want[kind], "clean " + name, exact=True if kind == "epochs" else None)
    return res


@pytest.mark.parametrize("place", xi.PLACES)
@pytest.mark.parametrize("kind", xi.POISONS)
@pytest.mark.parametrize("numerics", NUMERICS)
def test_a_poisoned_float32_epoch(ctxs, clean_float, tmp_path, numerics, kind, place):
    ctx = ctxs[numerics]
    rec7, pos = xi.float_recording(), xi.positions(xi.N_A)
    for slot in xi.SLOTS:
        what = f"{kind} in {place} of epoch {slot}"
        want = poisoned_want(kind, place, slot)
        got = float_paths(ctx, xi.poison(rec7, pos[slot], kind, place), pos, tmp_path, f"s{slot}")
        for name, (g, k) in got.items():
            check(ctx, g, want[k], f"{what}: {name}", exact=True if k == "epochs" else None)
            isolated(ctx, g, clean_float[numerics][name][0], {slot}, f"{what}: {name}")
        # E: a clean launch on the same context after the poisoned ones
        rec3 = np.ascontiguousarray(rec7[:, :3])
        check(ctx, ctx.process_recording(rec3, 3, xi.COLS3, xi.RES3, pos),
              clean_want()["rows3"], f"clean launch after {what}")
        counters_sane(ctx)


@pytest.mark.parametrize("kind", xi.MAGNITUDES)
@pytest.mark.parametrize("numerics", NUMERICS)
def test_b_float32_magnitudes(ctxs, tmp_path, numerics, kind):
    ctx = ctxs[numerics]
    rec7, pos = xi.float_magnitude(kind), xi.positions(xi.N_A)
    want = float_wants(rec7, pos)
    for name, (g, k) in float_paths(ctx, rec7, pos, tmp_path, kind).items():
        check(ctx, g, want[k], f"{kind}: {name}", exact=True if k == "epochs" else None)
    counters_sane(ctx)


# ---- C: int16 recordings with edge resolutions ---------------------------------------------------
def int16_paths(ctx, name):
    """window_kernel (3 of 3), any-layout (ct = 5), window_c32_kernel (32 of 32, 9 epochs), one-pass
    and streamed -> [(what, run, want)]; the oracle's results are computed once per call."""
    kind = xi.RES_SETS[name][1]
    raw3, pos = xi.int16_recording(xi.N_A, 3, kind), xi.positions(xi.N_A)
    res3 = xi.res_for(name, 3)
    want3 = oracle.process_recording(raw3, [0, 1, 2], res3, pos)
    ep3 = oracle.decode_epochs(raw3, [0, 1, 2], res3, pos)
    raw5 = xi.int16_recording(xi.N_A, 5, kind)
    want5 = oracle.process_recording(raw5, [4, 0, 2], res3, pos)
    raw32, pos9, res32 = xi.int16_recording(9, 32, kind), xi.positions(9), xi.res_for(name, 32)
    want32 = oracle.process_recording(raw32, list(range(32)), res32, pos9)
    return {
        "window": (lambda: ctx.process_recording(raw3, 3, [0, 1, 2], res3, pos), want3),
        "any_layout": (lambda: ctx.process_recording(raw5, 5, [4, 0, 2], res3, pos), want5),
        "c32": (lambda: ctx.process_recording(raw32, 32, list(range(32)), res32, pos9), want32),
        "one_pass": (lambda: ctx.process_recording_epochs(raw3, 3, [0, 1, 2], res3, pos), (want3, ep3)),
        "streamed": (lambda: ctx.process_recording_streamed(raw3, 3, [0, 1, 2], res3, pos,
                                                            chunk_frames=4099), want3),
    }


@pytest.mark.parametrize("name", list(xi.RES_SETS))
@pytest.mark.parametrize("numerics", NUMERICS)
def test_c_int16_edge_resolutions(ctxs, numerics, name):
    ctx = ctxs[numerics]
    paths = int16_paths(ctx, name)

    def run(which, tag):
        fn, want = paths[which]
        got = fn()
        if which == "one_pass":
            check(ctx, got[0], want[0], f"{name}: one_pass rows{tag}")
            check(ctx, got[1], want[1], f"{name}: one_pass epochs{tag}", exact=True)
        else:
            check(ctx, got, want, f"{name}: {which}{tag}")

    for which in paths:
        run(which, "")
    # the same after launches that sent half of their rows to the guard's second stage: under fma
    # the 3-channel and the 32-channel window kernels then run their tracking variants, which
    # decode the edge resolutions too (under EXACT this only repeats the launch)
    for which, ct, n in (("window", 3, xi.N_A), ("c32", 32, 9)):
        flat, fpos = xi.flat_recording(n, ct)
        cols, res = list(range(ct)), [0.1] * ct
        fwant = oracle.process_recording(flat, cols, res, fpos)
        before = ctx.guard_detail()[1]
        for i in range(2):
            check(ctx, ctx.process_recording(flat, ct, cols, res, fpos), fwant, f"flat {ct} #{i}")
        if numerics == "fma":
            assert ctx.guard_detail()[1] - before >= 2 * ((n + 1) // 2)   # > 1/16 of the rows
        for i in range(2):
            run(which, f" after flat launches #{i}")
    counters_sane(ctx)


# ---- D: double epochs ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", xi.D_SHAPES)
@pytest.mark.parametrize("numerics", NUMERICS)
def test_d_scaled_double_epochs_device(ctxs, numerics, n, C):
    import torch
    ctx = ctxs[numerics]
    ep = xi.double_epochs(n, C)

    def run(x):
        got = ctx.extract_features(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        ctx.synchronize()
        return got.cpu().numpy()

    want = oracle.extract_features(ep)
    base = run(ep)
    check(ctx, base, want, f"unscaled n={n} C={C}")
    for k in xi.K_INVARIANT:
        got = run(xi.scaled(ep, k))
        check(ctx, got, want, f"2^{k} n={n} C={C}")   # the oracle's rows are those of k = 0
        if numerics == "exact":
            assert np.array_equal(bits(got), bits(base)), f"EXACT rows change with the scale 2^{k}"
    for k in (xi.K_OVERFLOW, xi.K_UNDERFLOW):
        s = xi.scaled(ep, k)
        want_k = oracle.extract_features(s)
        redone = ctx.guard_detail()[2]
        got = run(s)
        check(ctx, got, want_k, f"2^{k} n={n} C={C}")
        if numerics == "fma":
            # the guard sends a row whose sum of squares left [2^-969, 2^1023] to EXACT (guard.h):
            # every row at 2^-530 (squares ~2^-1040), the overflowed (all-zero) rows at 2^505
            redone = ctx.guard_detail()[2] - redone
            gone = n if k == xi.K_UNDERFLOW else int((~want_k.any(axis=1)).sum())
            assert gone <= redone <= n, (k, gone, redone)
            if gone == n:
                check(ctx, got, want_k, f"2^{k} n={n} C={C}: recomputed rows", exact=True)
    bad, where = xi.poisoned_epochs(ep)
    got = run(bad)
    check(ctx, got, oracle.extract_features(bad), f"poisoned n={n} C={C}")
    isolated(ctx, got, base, set(where), f"poisoned n={n} C={C}")
    check(ctx, run(ep), want, f"clean launch after the poisoned one n={n} C={C}")   # E
    counters_sane(ctx)


@pytest.mark.parametrize("numerics", NUMERICS)
def test_d_per_epoch_host_call_mailbox_off_and_on(numerics):
    """IFeatureExtraction.extractFeatures one epoch at a time from host memory: EXACT rows in both
    numerics, by a launch per call and by the resident server (a host-only context of its own)."""
    n, C = 9, 3
    ep = xi.double_epochs(n, C)
    bad, where = xi.poisoned_epochs(ep)
    inputs = [("unscaled", ep)] + [(f"2^{k}", xi.scaled(ep, k))
                                   for k in xi.K_INVARIANT + (xi.K_OVERFLOW, xi.K_UNDERFLOW)]
    inputs.append(("poisoned", bad))
    wants = {tag: oracle.extract_features(x) for tag, x in inputs}
    for k in xi.K_INVARIANT:
        assert np.array_equal(bits(wants[f"2^{k}"]), bits(wants["unscaled"]))
    c = fx.Context(0, numerics=numerics)
    try:
        for mailbox in (False, True):
            c.set_mailbox(mailbox)
            rows = {}
            for tag, x in inputs:
                x = np.ascontiguousarray(x)
                rows[tag] = np.stack([c.extract_features(x[i:i + 1])[0] for i in range(n)])
                check(c, rows[tag], wants[tag], f"per-epoch {tag} mailbox={mailbox}", exact=True)
            isolated(c, rows["poisoned"], rows["unscaled"], set(where), f"per-epoch mailbox={mailbox}")
        c.set_mailbox(False)
        counters_sane(c)
    finally:
        c.set_mailbox(False)
        c.close()


# ---- E: the adaptive strategy and the counters after NaN rows ------------------------------------
def test_e_guard_state_survives_nan_rows():
    """NaN rows in more than 1/16 of a launch (float32 samples, then int16 overflow), each followed
    by clean int16 launches on the same fma context -- the first of them picks its strategy from
    the counters the poisoned launch left: still the oracle's rows, and the counters stay ordered,
    also across a reset."""
    c = fx.Context(0, numerics="fma")
    try:
        pos = xi.positions(xi.N_A)
        clean = xi.int16_recording(xi.N_A, 3, "moderate")
        want = oracle.process_recording(clean, [0, 1, 2], [0.1] * 3, pos)
        rec3 = np.ascontiguousarray(xi.float_recording()[:, :3])
        for e in (1, 4, 9, 12):
            rec3 = xi.poison(rec3, pos[e], "nan", "window")
        spikes = xi.int16_recording(xi.N_A, 3, "full_scale")
        poisoned = [
            ("float32 NaN", lambda: c.process_recording(rec3, 3, xi.COLS3, xi.RES3, pos),
             oracle.process_recording(rec3, xi.COLS3, xi.RES3, pos), 4),
            ("int16 overflow", lambda: c.process_recording(spikes, 3, [0, 1, 2], [2e34] * 3, pos),
             oracle.process_recording(spikes, [0, 1, 2], [2e34] * 3, pos), 3),
        ]
        for what, run, pwant, nbad in poisoned:
            for reset in (False, True):
                got = run()
                check(c, got, pwant, what)
                assert int(np.isnan(got).all(axis=1).sum()) == nbad
                counters_sane(c)
                checked, rechecked, redone = c.guard_detail(reset=reset)
                assert redone >= nbad, (what, checked, rechecked, redone)
                for i in range(3):
                    check(c, c.process_recording(clean, 3, [0, 1, 2], [0.1] * 3, pos), want,
                          f"clean launch #{i} after {what}")
                    counters_sane(c)
        c.guard_detail(reset=True)
        assert c.guard_detail() == (0, 0, 0)
    finally:
        c.close()
