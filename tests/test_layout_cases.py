"""tests/layout_cases.py off the GPU: every newly restated constant and
rule is the one in the sources (read with regular expressions, so a changed limit fails here and
moves its case instead of silently un-testing it), every case takes the kernels, chunk count and
LDS bytes it names on the restatements alone, every edge pair lies on either side of its
predicate, every kernel with a dynamic allocation has a case within 512 B of its limit, and every
case's input gives the oracle finite rows with the null-space rows where they are named.
tests/test_gpu_layout_edges.py runs the device at exactly these layouts."""
import re

import numpy as np
import pytest

import layout_cases as L
import refusal_cases as R
from oracle import oracle
from test_refusal_cases import body, ints, source


def ids(cases):
    return [c.name for c in cases]


# ---- the restated rules are the sources' ----------------------------------------------------------
def test_cut_chunk_frames_is_the_sources():
    k = source("cut.hip")
    chunk = body(k, "static int cut_chunk_frames(")
    assert "for (int nch = 1;; ++nch) {" in chunk
    assert "const int nfc = ((dev::kPost + nch - 1) / nch + 1) & ~1;" in chunk
    assert "if ((int64_t)nfc * frame_bytes + slack <= dev::kCutLdsMax || nfc <= 2) return nfc;" in chunk
    assert "constexpr int kCutLdsMax = EEGFX_CUT_LDS_MAX;" in k
    impl = body(k, "static hipError_t cut_epochs_impl(")
    for line in ("const int nfc = cut_chunk_frames(fbytes, 8);",
                 "const int fs_bytes = (fbytes / 4 + 1) * 4;",
                 "const int nfc = cut_chunk_frames(fs_bytes, 0);",
                 "(size_t)nfc * fbytes + 8, st,", "const size_t lds = (size_t)nfc * fs_bytes;"):
        assert line in impl, line
    assert impl.count("const int nchunks = (dev::kPost + nfc - 1) / nfc;") == 2
    one = body(k, "static hipError_t cut_features_impl(")
    assert "dev::staged_features_lds((size_t)dev::kPost * fbytes + 8, C)" in one
    assert "dev::staged_features_lds((size_t)dev::kPost * fs_bytes, C)" in one
    # by hand: 750 frames in one chunk, 376 in two, 250 in three, 188 in four
    assert [L.cut_chunk_frames(fs, 0) for fs in (84, 88, 176, 264)] == \
        [(750, 1), (376, 2), (250, 3), (188, 4)]
    assert L.cut_chunk_frames(174, 8) == (376, 2) and 376 * 174 + 8 == 65432
    assert L.cut_chunk_frames(10 ** 6, 0) == (2, 375)


def test_the_two_rule_and_the_wide_launch_are_the_sources():
    wide = source("wide.hip")
    # the definition (a declaration precedes launch_window_wide)
    kernels = body(wide[wide.rindex("static hipError_t launch_window_wide_kernels("):],
                   "static hipError_t launch_window_wide_kernels(")
    assert ints(r"const bool two = wide_lds_per_epoch\(fmt, ct, C\) <= (\d+) \* 1024;", kernels) == \
        (L.WIDE_TWO_MAX // 1024,)
    assert "return two ? launch_wide_t<T, FA, 2>(" in kernels and ": launch_wide_t<T, FA, 1>(" in kernels
    assert "if (fmt == 0 && ct == 32 && !two) {  // the frame size as a compile-time constant" in kernels
    assert kernels.count("launch_wide_t<int16_t, true, 1, 64") == 2
    assert kernels.count("launch_wide_t<int16_t, false, 1, 64") == 2
    assert kernels.index("ct == 32 && C == 32 && ((uintptr_t)out & 15) == 0") < \
        kernels.index("ct == 32 && !two")
    launch = body(wide, "hipError_t launch_wide_t(")
    assert "const size_t lds = (size_t)EPW * 8 * (4 * FB + 1) * 16 + (size_t)EPW * 16 * C * 8 + " \
           "EPW * 8 +\n                     (FAST ? (size_t)EPW * C * 8 : 0);" in launch
    assert "const dim3 grid((unsigned)((n + EPW - 1) / EPW));" in launch
    # the non-temporal variants (the sparse inputs select them)
    assert "fmt == 0 && streaming_reads(n_frames, n, dev::kPre + 687)" in wide
    assert wide.count("streaming_reads(n_frames, n, dev::kWin + 8)") == 2
    assert "return n > 0 && n_frames / n >= min_spacing;" in source("fused.hip")
    # the follow-up launch of the guard
    g = source("guard.hip")
    assert ints(r"constexpr int kGuardGrid = (\d+);", g) == (L.GUARD_GRID,)
    assert ints(r"constexpr int kGuardBlock = (\d+);", g) == (L.GUARD_BLOCK,)
    assert "for (int c0 = 8 * w; c0 < C; c0 += SIG) {" in g
    assert "for (int i = blockIdx.x; i < cnt; i += gridDim.x) {" in g
    # by hand: the issue's 65,056 B of 65,536
    assert L.window_variant(R.INT16, 63, 3, True) == ("window_wide_kernel", 1, 0, 65056)
    assert L.window_variant(R.INT16, 31, 3, True)[1:3] == (2, 0)
    assert L.window_variant(R.INT16, 32, 3, True)[1:3] == (1, 64)


def test_rows_out_and_the_small_batches_are_the_sources():
    k = source("extract.hip")
    impl = body(k, "static hipError_t features_from_epochs_impl(")
    assert "const size_t lds_rows = dev::kFeWinBytes + sizeof(double) * (8 * (size_t)C * nfeat + 8);" in impl
    assert ints(r"const bool rows_out = 3 \* lds_rows > (\d+) \* 1024;", impl) == (L.FE_CU_LDS // 1024,)
    assert "sizeof(double) * (rows_out ? 8 * 16 + 8 : 8 * (size_t)C * nfeat + 8);" in impl
    assert "dim3 grid((unsigned)((n + 7) / 8)), block(64);" in impl
    assert "constexpr int kFeSeg = kSegLen + 1;" in k and "constexpr int kFeWin = 8 * kFeSeg;" in k
    assert "constexpr size_t kFeWinBytes = sizeof(double) * 8 * kFeWin;" in k
    dwt = source("dwt8.h")
    assert ints(r"constexpr int kWin = (\d+);", dwt) == (L.WIN,)
    assert "constexpr int kSegLen = kWin / kLanesPerSignal;" in dwt
    assert ints(r"constexpr int kLanesPerSignal = (\d+);", dwt) == (8,)
    assert L.FE_WIN_BYTES == 8 * 8 * 8 * (L.WIN // 8 + 1) == 33280
    small = source("small.hip")
    assert ints(r"constexpr int kSmallMaxC = (\d+);", small) == (L.SMALL_MAX_C,)
    assert "return C >= 1 && C <= dev::kSmallMaxC;" in body(small, "bool features_small_supported(")
    api = source("api.cpp")
    assert ints(r"constexpr size_t kZeroCopyBytes = \(size_t\)(\d+) << (\d+);", api) == (768, 10)
    assert "(size_t)n * C * row_w <= kZeroCopyBytes && features_small_supported(C) &&" in api
    # the issue's edges, by hand
    assert [L.rows_out(C, f) for f, C in ((16, 20), (16, 21), (8, 41), (8, 42), (12, 27), (12, 28))] \
        == [False, True] * 3


def test_static_shared_declarations_are_the_ones_counted():
    """The bytes a kernel declares on top of its dynamic allocation."""
    def shared(text):
        return sorted(re.findall(r"^\s*(?:extern )?__shared__ (.*);", text, re.M))

    wide, k = source("wide.hip"), source("cut.hip")
    assert shared(body(wide, "void baseline_any_kernel(")) == \
        ["__attribute__((aligned(16))) uint8_t smem[]", "int64_t sB[256]"]
    assert shared(body(wide, "void window_wide_kernel(")) == \
        ["__attribute__((aligned(16))) uint8_t smem[]"]
    for head in ("void cut_write_lds_kernel(", "void cut_write_lds_packed_kernel("):
        assert shared(body(k, head)) == \
            ["__attribute__((aligned(16))) uint32_t stage[]", "float s_res[kMaxChannels], s_base[kMaxChannels]",
             "int s_col[kMaxChannels]"], head
    assert shared(body(source("extract.hip"), "void features_from_epochs_kernel(")) == \
        ["__attribute__((aligned(16))) double fsmem[]", "__attribute__((aligned(16))) double win[8 * kFeWin]"]
    assert L.STATIC == {"baseline_any_kernel": 2048, "cut_write_lds_kernel": 768,
                        "cut_write_lds_packed_kernel": 768, "window_wide_kernel": 0,
                        "features_from_epochs_kernel": 33280}
    assert R.MAX_CHANNELS == 64
    # every bound is on the dynamic bytes alone
    assert "EB * bstq * 16 <= 64 * 1024;" in body(wide, "bool baseline_any_supported(")
    assert "dev::staged_features_lds(stage, C) <= 64 * 1024" in body(k, "static bool cut_features_fit(")


def test_the_route_taken_with_a_shifted_out():
    """routes.cpp: the 3-of-3 kernels ask for an aligned `out`, then wide_supported decides."""
    routes = body(source("routes.cpp"), "void run_features_from_raw(")
    assert routes.index("if (fused_supported(fmt, ct, C, out)) {") < \
        routes.index("if (wide_supported(fmt, ct, C)) {") < routes.index("launch_cut_epochs(")
    assert "HIP_CHECK(launch_baseline_any(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, fscratch," \
        in routes
    assert L.features_kernels(R.INT16, 3, 3) == ("baseline_kernel", 64, "window_kernel")
    assert L.features_kernels(R.INT16, 3, 3, False) == ("baseline_any_kernel", 85, "window_wide_kernel")
    assert L.features_kernels(R.INT16, 32, 32, False)[2] == "window_wide_kernel"
    assert L.features_kernels(R.INT16, 32, 31, False) == L.features_kernels(R.INT16, 32, 31)


# ---- every case is what it names ------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES, ids=ids(L.CASES))
def test_each_case_takes_the_named_kernels_and_lds(case):
    got = L.launches(case)
    assert tuple(l.kernel for l in got) == case.kernels
    assert tuple(l.dyn for l in got) == case.dyn
    fma = tuple(l.dyn_fma for l in got)
    assert (fma if fma != case.dyn else None) == case.dyn_fma
    assert 2 <= case.C <= R.MAX_CHANNELS and (case.dtype is None or case.C <= case.ct)
    for l in got:
        if l.dyn is not None:
            assert l.kernel in L.STATIC and l.dyn_fma <= L.LIMIT_64K
    if case.entry in ("features", "one_pass", "cut"):
        tile = L.tile_of(case)
        if case.nulls == L.NULLS_GUARD:      # the guard's follow-up: more flagged rows than its grid
            assert case.n == L.N_GUARD > case.nulls > L.GUARD_GRID and case.C > 16
            assert L.guard_follow_up(case) and case.n >= 2 * tile + 2
        else:
            assert case.n == min(2 * tile + 2, 24), tile
            # but for the 3-of-3 layout (tiles of 64 and 85, tested at their edges by
            # test_gpu_refused_positions.py), two tiles and a ragged third
            assert case.n == 2 * tile + 2 or (case.ct, case.C) == (3, 3)
        cols, res = L.selection(case)
        assert cols[0] == case.ct - 1 and cols[-1] == 0 and len(res) == case.C
    elif case.entry == "extract":
        assert case.n == 2 * 8 + 2
    else:
        assert case.n in (1, 4) and case.n * case.C * L.WIN * 8 <= L.ZERO_COPY_BYTES


def test_case_names_are_distinct_and_every_entry_is_met():
    assert len(L.BY_NAME) == len(L.CASES)
    assert {c.entry for c in L.CASES} == {"features", "one_pass", "cut", "extract", "small"}
    seen = {l.kernel for c in L.CASES for l in L.launches(c)}
    assert seen == {"baseline_kernel", "window_kernel", "baseline_any_kernel", "window_wide_kernel",
                    "window_c32_kernel", "cut_write_lds_kernel", "cut_write_lds_packed_kernel",
                    "cut_write_small_kernel", "cut_write_kernel", "cut_epochs_kernel",
                    "features_from_epochs_kernel", "features_small_kernel"}
    variants = {(l.kernel, l.variant) for c in L.CASES for l in L.launches(c)}
    assert {("window_wide_kernel", "EPW=2"), ("window_wide_kernel", "EPW=1"),
            ("window_wide_kernel", "EPW=1 FBC=64"), ("features_from_epochs_kernel", "rows_out"),
            ("features_from_epochs_kernel", "rows_lds")} <= variants
    for kernel in ("cut_write_lds_kernel", "cut_write_lds_packed_kernel"):
        assert {v for k, v in variants if k == kernel} >= \
            {"chunks=1", "chunks=2", "chunks=3", "one-pass"}, kernel
    assert ("cut_write_lds_kernel", "chunks=4") in variants
    # float32 at one epoch a workgroup, the whole range's ends
    f32 = [c for c in L.CASES if c.dtype == L.F32 and c.kernels[-1] == "window_wide_kernel"]
    assert {c.ct for c in f32} >= {15, 16, 29, 31}


@pytest.mark.parametrize("a,b,pred", L.EDGES, ids=["%s|%s" % e[:2] for e in L.EDGES])
def test_each_edge_pair_lies_on_either_side_of_its_predicate(a, b, pred):
    ca, cb = L.BY_NAME[a], L.BY_NAME[b]
    va, vb = L.predicate(pred, ca), L.predicate(pred, cb)
    assert va != vb, (pred, va, vb)
    la, lb = L.launches(ca), L.launches(cb)
    assert [(l.kernel, l.variant) for l in la] != [(l.kernel, l.variant) for l in lb]
    assert (ca.entry, ca.dtype) == (cb.entry, cb.dtype)
    if pred in ("two", "wide_supported", "one_pass", "any_supported", "rows_out", "small_supported",
                "any_tile", "dword_frames"):
        # neighbours: nothing lies between the two layouts
        if ca.C == cb.C:
            assert abs(ca.ct - cb.ct) == 1, (ca.ct, cb.ct)
        else:
            assert abs(ca.C - cb.C) == 1 and abs(ca.ct - cb.ct) <= 1
    if pred == "chunks":            # the layouts between the two stay on one side or the other
        lo, hi = sorted((ca.ct, cb.ct))
        packed = lambda ct: R.frame_bytes(R.fmt_of(ca.dtype), ct) % 4 != 0
        for ct in range(lo + 1, hi):
            assert packed(ct) != packed(lo)      # the other staging (packed against whole dwords)


def test_lds_totals():
    """Every kernel with a dynamic allocation has a case within 512 B of its limit, and no
    workgroup asks for more than a gfx950 CU gives one (160 KB)."""
    rows, closest = [], {}
    for case in L.CASES:
        for l in L.launches(case):
            if l.dyn is None:
                continue
            total = l.dyn_fma + L.STATIC[l.kernel]
            rows.append((total, case.name, l.kernel, l.variant, l.dyn_fma, L.STATIC[l.kernel]))
            assert total <= L.LDS_PER_WORKGROUP
            assert l.dyn_fma <= L.LIMIT[l.kernel] or l.kernel == "features_from_epochs_kernel"
            gap = L.LIMIT[l.kernel] - l.dyn_fma
            if gap >= 0:
                closest[l.kernel] = min(closest.get(l.kernel, gap), gap)
    print("\n%-20s %-30s %-14s %8s %7s %8s" % ("case", "kernel", "variant", "dynamic", "static", "total"))
    for total, name, kernel, variant, dyn, static in sorted(rows, reverse=True):
        print("%-20s %-30s %-14s %8d %7d %8d%s" % (name, kernel, variant, dyn, static, total,
                                                   "  > 64 KB" if total > L.LIMIT_64K else ""))
    assert set(closest) == set(L.STATIC)
    for kernel, gap in closest.items():
        assert gap <= 512, (kernel, gap)
    over = {(name, kernel) for total, name, kernel, *_ in rows if total > L.LIMIT_64K}
    # the launches no earlier test made: static + dynamic above 64 KB
    assert {k for _, k in over} == {"baseline_any_kernel", "cut_write_lds_kernel",
                                    "cut_write_lds_packed_kernel"}
    assert max(t for t, *_ in rows) == 65440 + 2048 and ("c-i16-327x2", "baseline_any_kernel") in over
    assert ("o-i16-43x5", "cut_write_lds_packed_kernel") in over      # 65,040 + 768


# ---- the inputs, against the oracle alone ---------------------------------------------------------
RAW_CASES = [c for c in L.CASES if c.entry in ("features", "one_pass", "cut")]


def alternating(window):
    """Every row of [..., 512] is v, -v, v, ... for one v != 0."""
    return bool(np.all(window[..., 1:] == -window[..., :-1]) and np.all(window[..., 0] != 0))


@pytest.mark.parametrize("case", RAW_CASES, ids=ids(RAW_CASES))
def test_inputs_of_the_raw_cases(case):
    raw = L.recording(case.dtype, case.ct, L.null_frames(case))
    assert raw.shape == (L.N_FRAMES, case.ct) and raw.dtype == np.dtype(case.dtype)
    cols, res = L.selection(case)
    for pos, nulls in ((L.positions(case), L.n_nulls(case)), (L.sparse_positions(), 1)):
        if case.dtype != L.I16 and len(pos) == L.SPARSE_N:
            continue                                   # the non-temporal variants are int16's
        named = L.null_rows(case, pos)
        assert named.tolist() == list(range(nulls))
        ep = oracle.decode_epochs(raw, cols, res, pos)
        rows = oracle.process_recording(raw, cols, res, pos)
        assert np.isfinite(ep).all() and np.isfinite(rows[:-1]).all()
        for r in range(len(pos)):
            assert alternating(ep[r, :, 175:175 + L.WIN]) == (r in named), r
        assert {int(p) % 2 for p in pos} == {0, 1}
    fb = R.frame_bytes(R.fmt_of(case.dtype), case.ct)
    dense = L.positions(case)[:-1]
    phases = {int(p) * fb % 16 for p in dense}           # every 16-byte phase the frame size allows
    assert len(phases) == min(len(dense), 16 // np.gcd(16, L.SPACING * fb % 16))
    pos = L.positions(case)
    assert pos[-1] + L.POST - L.N_FRAMES == L.TAIL == 450
    ep = oracle.decode_epochs(raw, cols, res, pos)
    assert np.all(ep[-1, :, L.POST - L.TAIL:] == ep[-1, :, -1:])     # zero padding less the baseline


EPOCH_CASES = [c for c in L.CASES if c.entry in ("extract", "small")]


@pytest.mark.parametrize("case", EPOCH_CASES, ids=ids(EPOCH_CASES))
def test_inputs_of_the_epoch_cases(case):
    ep, nulls = L.epochs_input(case)
    assert ep.shape == (case.n, case.C, L.POST)
    rows = oracle.extract_features(ep, nfeat=case.nfeat)
    assert rows.shape == (case.n, case.C * case.nfeat) and np.isfinite(rows).all()
    assert [alternating(ep[r, :, 175:175 + L.WIN]) for r in range(case.n)] == \
        [r in nulls for r in range(case.n)]
    assert len(nulls) == (min(4, case.n - 1) if case.n > 1 else 0)
