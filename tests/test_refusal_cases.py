"""tests/refusal_cases.py off the GPU: every restated launch constant is the one in the sources
(read with regular expressions, so a changed cap or tile fails here and moves its case instead of
silently un-testing it), every named row falls in the tile position, trip and unroll slot its case
is named for, and every named layout reaches the named kernels, on the restatements alone
(DESIGN.md section 10.5).  The GPU tests run the device at exactly these placements."""
import os
import re

import numpy as np
import pytest

import refusal_cases as R


def source(name):
    return open(os.path.join(R.CSRC, name)).read()


def ints(pattern, text, flags=0):
    m = re.search(pattern, text, flags)
    assert m, pattern
    return tuple(int(g) for g in m.groups())


def body(text, head):
    """The text of the function whose definition starts with `head`, up to its closing brace in
    column 0."""
    start = text.index(head)
    return text[start:text.index("\n}", start)]


# ---- the restated constants are the sources' ------------------------------------------------------
def test_epoch_geometry_and_tiles():
    assert ints(r"constexpr int kPre = (\d+);", source("dwt8.h")) == (R.PRE,)
    assert ints(r"constexpr int kPost = (\d+);", source("dwt8.h")) == (R.POST,)
    assert ints(r"constexpr int kMaxChannels = (\d+);", source("launch.h")) == (R.MAX_CHANNELS,)
    fused = body(source("fused.hip"), "hipError_t launch_fused_baseline(")
    assert ints(r"constexpr int kTile = (\d+);", fused) == (R.BASELINE_TILE,)
    assert "(n + kTile - 1) / kTile" in fused
    assert "fmt == 0 && ct == 3 && C == 3 && ((uintptr_t)out & 15) == 0" in \
        body(source("fused.hip"), "bool fused_supported(")


def test_baseline_any_tile_and_the_wide_bound():
    wide = source("wide.hip")
    tile = body(wide, "static int baseline_any_tile(")
    assert ints(r"int EB = (\d+) / C;", tile) == (R.ANY_LANES,)
    assert ints(r"> (\d+) \* 1024\) --EB;", tile) == (R.ANY_LDS_TARGET // 1024,)
    assert "(dev::kPre * FB + 15) / 16 + 2" in tile
    assert ints(r"EB \* bstq \* 16 <= (\d+) \* 1024;",
                body(wide, "bool baseline_any_supported(")) == (R.ANY_LDS_MAX // 1024,)
    assert ints(r"wide_lds_per_epoch\(fmt, ct, C\) <= (\d+) \* 1024;",
                body(wide, "bool wide_supported(")) == (R.WIDE_LDS_MAX // 1024,)
    assert "(size_t)8 * (4 * FB + 1) * 16 + (size_t)16 * C * 8 + 8 + (size_t)C * 8" in \
        body(wide, "static size_t wide_lds_per_epoch(")
    assert "fmt == 0 && ct == 32 && C == 32 && ((uintptr_t)out & 15) == 0" in \
        body(wide, "static hipError_t launch_window_wide_kernels(")
    # the tiles of the layouts this project ships with, by hand: 6,432 B a 32-channel run
    assert R.baseline_any_tile(R.INT16, 32, 32) == (8, 402)
    assert R.baseline_any_tile(R.INT16, 5, 3) == (55, 65)


def test_writer_choice_constants():
    k = source("cut.hip")
    assert ints(r"constexpr int kCutPairs = (\d+);", k) == (R.CUT_PAIRS,)
    assert ints(r"constexpr int kCfEpochs = (\d+);", k) == (R.CF_EPOCHS,)
    assert ints(r"#define EEGFX_CUT_LDS_MAX \((\d+) \* 1024\)", k) == (R.CUT_LDS_MAX // 1024,)
    impl = body(k, "static hipError_t cut_epochs_impl(")
    for line in ("std::is_same<E, float>::value || ((uintptr_t)out & 15) == 0",
                 "if (!aligned) scratch = nullptr;",
                 "C * (dev::kPost / 2) <= 256 * dev::kCutPairs",
                 "(int64_t)dev::kPost * fbytes <= 2 * 6000LL * C",
                 "stage && fbytes % 4 != 0 && fmt == 0", "stage && fbytes % 4 == 0"):
        assert line in impl, line
    fit = body(k, "static bool cut_features_fit(")
    assert "dev::staged_features_lds(stage, C) <= 64 * 1024" in fit
    assert "(size_t)(16 * C + 768) * 8" in k and "+ 64 * 8 + 16;" in k


def test_grid_caps():
    launch = source("launch.h")
    for name, want in (("kGatherThreads", R.THREADS), ("kGatherUnroll", R.GATHER_UNROLL),
                       ("kGatherMaxBlocks", R.GATHER_BLOCKS), ("kConfusionThreads", R.THREADS)):
        assert ints(r"constexpr int %s = (\d+);" % name, launch) == (want,)
    flow = source("flow.hip")
    assert "grid_for(m * dv, kGatherThreads * kGatherUnroll, kGatherMaxBlocks)" in flow
    assert ints(r"grid_for\(n, kConfusionThreads \* (\d+), (\d+)\)", flow) == \
        (R.CONFUSION_UNROLL, R.CONFUSION_BLOCKS)
    assert ints(r"constexpr int U = (\d+);", body(flow, "void confusion_kernel(")) == \
        (R.CONFUSION_UNROLL,)
    lr = body(source("logreg.hip"), "hipError_t launch_lr_validate(")
    assert ints(r"\(n \+ (\d+)\) / (\d+);", lr) == (R.THREADS - 1, R.THREADS)
    assert ints(r"g > (\d+) \? (\d+) : g\)+,\s*dim3\((\d+)\)", lr) == \
        (R.LR_BLOCKS, R.LR_BLOCKS, R.THREADS)
    plan = source("plan.hip")
    grid = body(plan, "unsigned grid_for(int64_t n)")
    assert ints(r"\(n \+ (\d+)\) / (\d+);", grid) == (R.THREADS - 1, R.THREADS)
    assert ints(r"g > (\d+) \? (\d+) : g", grid) == (R.PLAN_BLOCKS, R.PLAN_BLOCKS)
    assert plan.count("dim3(grid_for(n)), dim3(256)") + plan.count("dim3(grid_for(m)), dim3(256)") == 3
    assert ints(r"dt_bin_kernel, dim3\(grid_for\(n \* d, (\d+) \* (\d+), (\d+)\)\), dim3\((\d+)\)",
                source("dtree.hip")) == (R.THREADS, R.BIN_PER_THREAD, R.BIN_BLOCKS, R.THREADS)
    assert (R.LR_TRIP, R.CONFUSION_TRIP, R.GATHER_TRIP, R.PLAN_TRIP) == \
        (1_048_576, 2_097_152, 2_097_152, 2_097_152)


def test_the_clamps_are_the_eleven_the_routes_are_written_for():
    """Nine clamps in the kernels that read a position again, two in the checkers.  A tenth
    needs a route of its own in refusal_cases.ROUTES.  cut.hip writes the expression once, in
    cut_position(), and each of its six kernels calls that; the other files hold copies."""
    clamp = re.compile(r"\? p0? : (?:\(int64_t\))?kPre")
    cut = source("cut.hip")
    for name, want in R.CLAMPS_PER_FILE.items():
        if name == "cut.hip":
            assert clamp.findall(cut) == clamp.findall(body(cut, "int64_t cut_position(")) \
                == ["? p0 : kPre"]
            assert len(re.findall(r"(?<!int64_t )cut_position\(", cut)) == want
        else:
            assert len(clamp.findall(source(name))) == want, name
    callers = [k for k, f in R.CLAMPS.items() if f == "cut.hip"]
    assert len(callers) == R.CLAMPS_PER_FILE["cut.hip"]
    for kernel in callers:
        assert body(cut, "void %s(" % kernel).count("cut_position(") == 1, kernel
    assert sum(R.CLAMPS_PER_FILE.values()) == len(R.CLAMPS) + 2
    assert "if (threadIdx.x == 0 && !ok && err)" in body(cut, "void cut_epochs_kernel(")


# ---- positions ------------------------------------------------------------------------------------
def route_ids():
    return [r.name for r in R.ROUTES]


@pytest.mark.parametrize("route", R.ROUTES, ids=route_ids())
def test_each_layout_reaches_the_named_kernels(route):
    lay = R.layouts()[route.layout]
    assert route.C <= len(lay.cols)
    assert R.restated_kernels(route) == route.kernels
    if route.entry == "features64":      # the materialised epochs are float32: always "aligned"
        assert R.features_route(R.fmt_of(lay.dtype), lay.ct, route.C)[2] == "window_wide_kernel"
    if route.entry == "one_pass":
        assert R.one_pass_writer(R.fmt_of(lay.dtype), lay.ct, route.C) is not None
    if route.shifted:
        assert route.epochs == ("float64",)       # float stores align themselves


def test_every_clamp_has_a_route_and_every_route_is_distinct():
    assert len(set(route_ids())) == len(R.ROUTES)
    second = {r.kernels[2] for r in R.ROUTES}
    assert second >= set(R.CLAMPS) - {"exact_rows_kernel"}
    # guard.hip's recomputation follows window_wide_kernel under fma alone
    assert any(r.kernels[2] == "window_wide_kernel" and "fma" in r.numerics for r in R.ROUTES)
    assert {r.kernels[0] for r in R.ROUTES} == \
        {"baseline_kernel", "baseline_any_kernel", "cut_epochs_kernel"}
    for entry, epochs in (("one_pass", R.F64_F32), ("cut", R.F64_F32)):
        writers = {r.kernels[2] for r in R.ROUTES if r.entry == entry and r.epochs == epochs}
        assert len(writers) >= 3, entry


def test_cut_epochs_kernel_is_reached_by_both_of_its_routes():
    by_name = {r.name: r for r in R.ROUTES}
    lay = R.layouts()[by_name["cut-fallback-layout"].layout]
    assert (R.fmt_of(lay.dtype), lay.ct) == (R.INT16, 400)
    assert R.PRE * R.frame_bytes(R.INT16, 400) > 64 * 1024       # one run is more than 64 KB
    assert not R.baseline_any_supported(R.INT16, 400, 2)
    assert R.cut_writer(R.INT16, 400, 2)[2] == "cut_epochs_kernel"
    # ... and a layout the staged kernels take, but for a double `out` 8 bytes off
    assert R.cut_writer(R.INT16, 3, 3)[2] == "cut_features_c3_kernel"
    assert R.cut_writer(R.INT16, 3, 3, out_aligned=False) == \
        ("cut_epochs_kernel", 1, "cut_epochs_kernel")
    assert by_name["cut-fallback-shifted"].shifted


@pytest.mark.parametrize("tile", sorted({r.kernels[1] for r in R.ROUTES}))
def test_placements_meet_the_tile_edges(tile):
    n = R.epochs_of(tile)
    at = [divmod(i, tile) for i in R.placements(tile)]
    if tile == 1:       # cut_epochs_kernel: a workgroup an epoch, the first, the second, the last
        assert at == [(0, 0), (1, 0), (3, 0)] and n == 4
    else:               # two full tiles and a ragged third of two epochs
        assert set(at) == {(0, 0), (0, tile - 1), (1, 0), (2, 1)}
        assert -(-n // tile) == 3 and n % tile == 2 and tile > 2
    pos = R.good_positions(n)
    assert pos[0] == R.PRE and pos[-1] + R.POST <= R.N_FRAMES + R.PRE
    assert {int(p) % 2 for p in pos} == {0, 1}
    assert R.null_space_rows(pos).tolist() == [0, 1, 2, 3][:min(4, n)]
    assert R.PRE + 175 + 512 <= R.NULL_FRAMES        # the cut an invalid position is given


def test_bad_position_values():
    assert R.BAD_POSITION == 99 and R.BAD_POSITION in R.BAD_VALUES
    assert all(not (v >= R.PRE and v - R.PRE <= R.N_FRAMES) for v in R.BAD_VALUES + [R.N_FRAMES + 101])
    assert {2 ** 62, -(2 ** 63), 2 ** 63 - 1} <= set(R.BAD_VALUES)     # (p +- k) * FB overflows
    robustness = open(os.path.join(R.TESTS, "test_gpu_robustness.py")).read()
    assert re.search(r"^BAD = (.*)$", robustness, re.M).group(1) == \
        "[99, 0, -1, -(10 ** 15), 10 ** 15, 2 ** 62, -(2 ** 63), 2 ** 63 - 1]"


# ---- rows -----------------------------------------------------------------------------------------
def test_label_rows_of_the_sgd_trainers():
    places = [R.lr_place(r, R.LR_N) for r in R.LR_ROWS]
    assert [(p.trip, p.block, p.thread) for p in places] == \
        [(0, 0, 0), (0, R.LR_BLOCKS - 1, 255), (1, 0, 0), (1, 1, 43)]
    assert R.LR_N == 1_048_876


def test_label_rows_of_the_confusion_counts():
    n = R.CONFUSION_SMALL_N
    assert R.blocks(n, R.THREADS * R.CONFUSION_UNROLL, R.CONFUSION_BLOCKS) == 1
    places = [R.confusion_place(r, n) for r in R.CONFUSION_SMALL_ROWS]
    assert [(p.trip, p.slot, p.thread) for p in places] == \
        [(0, 0, 255), (0, 1, 0), (0, 1, 255), (0, 2, 0), (0, 2, 255), (0, 3, 0), (0, 3, 231)]
    n = R.CONFUSION_BIG_N
    assert R.blocks(n, R.THREADS * R.CONFUSION_UNROLL, R.CONFUSION_BLOCKS) == R.CONFUSION_BLOCKS
    last = R.confusion_place(n - 1, n)
    assert (last.trip, last.slot, last.block, last.thread) == (1, 0, 2, 187)
    assert R.confusion_place(R.CONFUSION_TRIP - 1, n) == (0, 3, R.CONFUSION_BLOCKS - 1, 255)


def test_bad_rows_of_the_gather():
    for d, m in R.GATHER_SHAPES.items():
        dv = R.gather_pieces(d)
        assert dv == {1: 1, 4: 2}[d] and m * dv == R.GATHER_TRIP + 1000
        assert R.blocks(m * dv, R.THREADS * R.GATHER_UNROLL, R.GATHER_BLOCKS) == R.GATHER_BLOCKS
        first, second = (R.gather_place(r, m, d) for r in R.gather_bad_rows(m))
        assert first.trip == second.trip == 1 and first.slot == second.slot == 0
        assert (first.block, first.thread) != (second.block, second.thread)
        early = R.gather_place(R.GATHER_EARLY_ROW, m, d)
        assert (early.trip, early.slot, early.block) == (0, 0, 0)
        assert R.GATHER_EARLY_ROW < R.gather_bad_rows(m)[0] < R.gather_bad_rows(m)[1] == m - 1
    assert R.gather_pieces(4, aligned=False) == 4 and R.gather_pieces(3) == 3


def test_offenders_of_the_plan():
    for n, offenders in R.PLAN_CASES:
        assert all(0 <= i < n for i in offenders) and list(offenders) == sorted(offenders)
    n, (a, b) = R.PLAN_CASES[-1]
    assert n == R.PLAN_BIG_N and R.blocks(n, R.THREADS, R.PLAN_BLOCKS) == R.PLAN_BLOCKS
    pa, pb = R.plan_place(a, n), R.plan_place(b, n)
    assert pa.trip == pb.trip == 1 and pa.block != pb.block
    assert R.plan_place(R.PLAN_TRIP - 1, n).trip == 0
    small = [o for m, o in R.PLAN_CASES if m == R.PLAN_SMALL_N]
    assert small == [(0,), (13,), (13, 17)]           # 13 and 17: two lanes of one wave


def test_rows_of_the_tree_binning():
    n, d = R.TREE_N, R.TREE_D
    assert (n * d) % R.THREADS != 0 and R.blocks(n * d, R.THREADS * R.BIN_PER_THREAD, R.BIN_BLOCKS) == 1
    assert R.bin_place(0, 0, n, d) == (0, 0, 0, 0)
    assert R.bin_place(n - 1, 0, n, d) == (3, 0, 0, 242)          # the last label
    assert R.bin_place(n - 1, d - 1, n, d) == (3, 0, 0, 246)      # the last element
    # the sampled case: a row outside Spark's sample is seen by dt_bin_kernel alone
    from eeg_dataanalysispackage_amd import classification as clf
    import dtree_reference as D
    n, d = R.TREE_SAMPLED_N, R.TREE_SAMPLED_D
    assert n > D.required_samples(8) == 10000
    kept = clf.spark_sample(n, 10000 / n, 1, 0)
    out = np.setdiff1d(np.arange(n), kept)
    assert 0 < out.size < n and out[-1] > out[0]
    assert R.bin_place(int(out[-1]), d - 1, n, d).trip >= 1 > R.bin_place(int(out[0]), 1, n, d).trip
