"""Where the epoch kernels are tested at the first and the last layout of every dispatch bucket
(DESIGN.md section 10.6): raw recording -> baselines -> epochs -> dwt-8 rows (cut.hip, extract.hip,
small.hip, wide.hip, fused.hip, guard.hip, routed by routes.cpp).  Which kernel a call takes is decided by host-side
predicates on (sample type, channels in the file ct, selected channels C), the output's alignment
and the marker spacing, most of them an LDS-size formula compared with a limit.  tests/
refusal_cases.py restates most of those predicates; this module imports them, restates the three
it lacks (cut_chunk_frames, the `two` rule with the compile-time-frame-size branch, rows_out and
features_small_supported) and names, for every predicate, the last layout one side of it and the
first on the other, with the kernels, the chunk count and the LDS bytes each must take.  Not a test
module: tests/test_layout_cases.py pins the restatements to the sources and proves every case from
them; tests/test_gpu_layout_edges.py runs the device at exactly these layouts.
"""
from collections import namedtuple

import numpy as np

import refusal_cases as R
from refusal_cases import (INT16, FLOAT32, PRE, POST, baseline_any_tile, cut_writer,  # noqa: F401
                           features_route, frame_bytes, one_pass_writer, staged_features_lds,
                           wide_lds_per_epoch)

# ---- the restatements refusal_cases.py lacks ------------------------------------------------------
WIDE_TWO_MAX = 32 * 1024           # wide.hip launch_window_wide_kernels: two epochs a workgroup
FE_WIN_BYTES = 8 * 8 * 8 * 65      # extract.hip kFeWinBytes: 8 windows of 8 segments of 65 doubles
FE_CU_LDS = 160 * 1024             # extract.hip features_from_epochs_impl: 3 workgroups a CU
SMALL_MAX_C = 16                   # small.hip kSmallMaxC
ZERO_COPY_BYTES = 768 << 10        # api.cpp kZeroCopyBytes: the small host batches
WIN = 512                          # dwt8.h kWin
GUARD_GRID, GUARD_BLOCK = 16, 128  # guard.hip kGuardGrid, kGuardBlock
LDS_PER_WORKGROUP = 160 * 1024     # gfx950
LIMIT_64K = 64 * 1024

# Static __shared__ bytes of the kernels that also take a dynamic allocation.
STATIC = {
    "baseline_any_kernel": 256 * 8,                 # int64_t sB[256]
    "cut_write_lds_kernel": 3 * 64 * 4,             # s_col, s_res, s_base [kMaxChannels]
    "cut_write_lds_packed_kernel": 3 * 64 * 4,
    "window_wide_kernel": 0,
    "features_from_epochs_kernel": FE_WIN_BYTES,    # double win[8 * kFeWin]
}
# What each of those dynamic allocations is bounded by (static bytes on top, except the batch
# extract, whose bound is a third of a CU for static + dynamic together).
LIMIT = {
    "baseline_any_kernel": R.ANY_LDS_MAX, "cut_write_lds_kernel": R.CUT_LDS_MAX,
    "cut_write_lds_packed_kernel": R.CUT_LDS_MAX, "window_wide_kernel": R.WIDE_LDS_MAX,
    "features_from_epochs_kernel": FE_CU_LDS // 3 - FE_WIN_BYTES,
}


def cut_chunk_frames(frame_bytes_, slack):
    """cut.hip cut_chunk_frames: (frames a chunk, chunks) of the staged write passes."""
    nch = 1
    while True:
        nfc = ((POST + nch - 1) // nch + 1) & ~1
        if nfc * frame_bytes_ + slack <= R.CUT_LDS_MAX or nfc <= 2:
            return nfc, -(-POST // nfc)
        nch += 1


def wide_two(fmt, ct, C):
    """wide.hip launch_window_wide_kernels: two epochs a workgroup while both fit 64 KB."""
    return wide_lds_per_epoch(fmt, ct, C) <= WIDE_TWO_MAX


def window_variant(fmt, ct, C, fast, out_aligned=True):
    """(kernel, epochs a workgroup, compile-time frame bytes or 0, dynamic LDS) of the window
    launch of a layout wide_supported takes (wide.hip launch_window_wide_kernels, launch_wide_t)."""
    if fmt == INT16 and ct == 32 and C == 32 and out_aligned:
        return "window_c32_kernel", 1, 64, 0
    two = wide_two(fmt, ct, C)
    epw = 2 if two else 1
    fbc = 64 if fmt == INT16 and ct == 32 and not two else 0
    fb = frame_bytes(fmt, ct)
    lds = epw * 8 * (4 * fb + 1) * 16 + epw * 16 * C * 8 + epw * 8 + (epw * C * 8 if fast else 0)
    return "window_wide_kernel", epw, fbc, lds


def features_kernels(fmt, ct, C, out_aligned=True):
    """refusal_cases.features_route, and the two layouts with kernels of their own (fused.hip
    fused_supported, the 32-of-32 montage) when `out` is 8 bytes off a 16-byte boundary."""
    own = R.is_c3(fmt, ct, C) or (fmt == INT16 and ct == 32 and C == 32)
    if out_aligned or not own:
        return features_route(fmt, ct, C)
    return "baseline_any_kernel", baseline_any_tile(fmt, ct, C)[0], "window_wide_kernel"


def rows_out(C, nfeat):
    """extract.hip features_from_epochs_impl: the rows leave through `out`, not LDS."""
    return 3 * (FE_WIN_BYTES + 8 * (8 * C * nfeat + 8)) > FE_CU_LDS


def extract_lds(C, nfeat):
    return 8 * (8 * 16 + 8 if rows_out(C, nfeat) else 8 * C * nfeat + 8)


def features_small_supported(C):
    return 1 <= C <= SMALL_MAX_C


def stage_rule(fmt, ct, C):
    """cut.hip cut_epochs_impl `stage`: staged frames at most twice the rows written."""
    return POST * frame_bytes(fmt, ct) <= 2 * 6000 * C


def small_rule(C):
    return C * (POST // 2) <= R.THREADS * R.CUT_PAIRS


def one_pass_stage_bytes(fmt, ct):
    fb = frame_bytes(fmt, ct)
    return POST * fb + 8 if fb % 4 != 0 else POST * ((fb // 4 + 1) * 4)


# ---- what a case launches -------------------------------------------------------------------------
# kernel, dynamic LDS bytes under exact and under fma numerics (None: none asked), and a word on
# the variant: "EPW=2", "FBC=64", "chunks=3", "rows_out", "rows_lds"
Launch = namedtuple("Launch", "kernel dyn dyn_fma variant")


def _baseline(fmt, ct, C, any_layout=False):
    """The baselines of the staged routes; any_layout: routes.cpp's wide branch, which takes
    baseline_any_kernel for the 3-of-3 layout too."""
    chk = R.checker(fmt, ct, C)
    if chk is None:
        return []
    if chk[0] == "baseline_kernel" and not any_layout:
        return [Launch("baseline_kernel", None, None, "")]
    eb, bstq = baseline_any_tile(fmt, ct, C)
    return [Launch("baseline_any_kernel", eb * bstq * 16, eb * bstq * 16, "EB=%d" % eb)]


def _cut(fmt, ct, C, out_aligned=True):
    writer = cut_writer(fmt, ct, C, out_aligned)[2]
    fb = frame_bytes(fmt, ct)
    base = _baseline(fmt, ct, C) if writer != "cut_epochs_kernel" else []
    if writer == "cut_write_lds_packed_kernel":
        nfc, nch = cut_chunk_frames(fb, 8)
        return base + [Launch(writer, nfc * fb + 8, nfc * fb + 8, "chunks=%d" % nch)]
    if writer == "cut_write_lds_kernel":
        fs = (fb // 4 + 1) * 4
        nfc, nch = cut_chunk_frames(fs, 0)
        return base + [Launch(writer, nfc * fs, nfc * fs, "chunks=%d" % nch)]
    return base + [Launch(writer, None, None, "")]


def _extract(C, nfeat):
    lds = extract_lds(C, nfeat)
    return [Launch("features_from_epochs_kernel", lds, lds,
                   "rows_out" if rows_out(C, nfeat) else "rows_lds")]


def launches(case):
    """The kernels of one call of the case's entry on aligned device buffers (a `shifted` case:
    the features' `out` 8 bytes off), in launch order; the guard's follow-up launch apart."""
    fmt, ct, C = R.fmt_of(case.dtype) if case.dtype else None, case.ct, case.C
    if case.entry == "features":
        route = features_kernels(fmt, ct, C, not case.shifted)
        if route[2] == "window_kernel":
            return [Launch("baseline_kernel", None, None, ""), Launch("window_kernel", None, None, "")]
        if R.wide_supported(fmt, ct, C):
            k, epw, fbc, lds = window_variant(fmt, ct, C, False, not case.shifted)
            lds_fma = window_variant(fmt, ct, C, True, not case.shifted)[3]
            word = "EPW=%d" % epw + (" FBC=%d" % fbc if fbc else "")
            return _baseline(fmt, ct, C, True) + [Launch(k, lds or None, lds_fma or None, word)]
        return _cut(fmt, ct, C) + _extract(C, 16)     # the scratch epochs are doubles, aligned
    if case.entry == "one_pass":
        one = one_pass_writer(fmt, ct, C)
        if one is None:
            return _cut(fmt, ct, C) + _extract(C, 16)
        if one[2] == "cut_features_c3_kernel":
            return _baseline(fmt, ct, C) + [Launch(one[2], None, None, "")]
        lds = staged_features_lds(one_pass_stage_bytes(fmt, ct), C)
        return _baseline(fmt, ct, C) + [Launch(one[2], lds, lds, "one-pass")]
    if case.entry == "cut":
        return _cut(fmt, ct, C)
    if case.entry == "extract":
        return _extract(C, case.nfeat)
    assert case.entry == "small"
    if case.n * C * WIN * 8 <= ZERO_COPY_BYTES and features_small_supported(C):
        return [Launch("features_small_kernel", None, None, "")]
    return _extract(C, case.nfeat)


def guard_follow_up(case):
    """Under fma numerics launch_window_wide follows window_wide_kernel with exact_rows_kernel."""
    return case.entry == "features" and launches(case)[-1].kernel == "window_wide_kernel"


def tile_of(case):
    """Epochs a workgroup of the kernel that reads the positions first."""
    if case.entry in ("extract", "small"):
        return 8                                           # features_from_epochs_kernel
    first = launches(case)[0]
    if first.kernel == "baseline_kernel":
        return R.BASELINE_TILE
    if first.kernel == "baseline_any_kernel":
        return baseline_any_tile(R.fmt_of(case.dtype), case.ct, case.C)[0]
    return 1


# ---- the cases ------------------------------------------------------------------------------------
# entry: "features" process_recording, "one_pass" process_recording_epochs, "cut" cut_epochs,
# "extract" extract_features on device epochs, "small" extract_features on host epochs.
# kernels / dyn: the kernels of a call in launch order and the dynamic LDS bytes of each (exact
# numerics; `dyn_fma` where fma asks for another size), None where the kernel asks for none.
# n: epochs of the dense input (2 T + 2 of the baseline tile T unless noted).  nulls: rows in the
# filters' null space.  shifted: a features `out` 8 bytes off a 16-byte boundary.
Case = namedtuple("Case", "name entry dtype ct C edge kernels dyn dyn_fma n nulls shifted nfeat",
                  defaults=(None, 24, 4, False, 16))
I16, F32 = "int16", "float32"
BA, WW, C32K = "baseline_any_kernel", "window_wide_kernel", "window_c32_kernel"
LDS, PACKED = "cut_write_lds_kernel", "cut_write_lds_packed_kernel"
SMALLW, DIRECT, FALLBACK = "cut_write_small_kernel", "cut_write_kernel", "cut_epochs_kernel"
FFE, FSMALL = "features_from_epochs_kernel", "features_small_kernel"
N_GUARD, NULLS_GUARD = 24, 20      # (33,33), (56,56): a second trip of exact_rows_kernel's grid


def _c(name, entry, dtype, ct, C, edge, kernels, dyn, **kw):
    return Case(name, entry, dtype, ct, C, edge, tuple(kernels), tuple(dyn), **kw)


CASES = [
    # ---- process_recording: the window kernels -----------------------------------------------------
    _c("f-i16-31x3", "features", I16, 31, 3, "two: last int16 layout at two epochs a workgroup",
       (BA, WW), (56160, 64528), dyn_fma=(56160, 64576), n=20),
    _c("f-i16-32x3", "features", I16, 32, 3, "two: first at one epoch, compile-time frame size",
       (BA, WW), (51456, 33288), dyn_fma=(51456, 33312), n=18),
    _c("f-i16-63x3", "features", I16, 63, 3, "wide_supported: last int16 ct at C = 3",
       (BA, WW), (50560, 65032), dyn_fma=(50560, 65056), n=10),
    _c("f-i16-64x3", "features", I16, 64, 3, "wide_supported: first refused, cut + extract",
       (BA, SMALLW, FFE), (51328, None, 3136), n=10),
    _c("f-i16-59x32", "features", I16, 59, 32, "wide_supported: last ct at C = 32",
       (BA, WW), (47360, 64648), dyn_fma=(47360, 64904), n=10),
    _c("f-i16-60x32", "features", I16, 60, 32, "wide_supported: first refused at C = 32",
       (BA, LDS, FFE), (48128, 46624, 1088), n=10),
    _c("f-i16-56x56", "features", I16, 56, 56, "wide_supported: last square int16 layout",
       (BA, WW), (44928, 64648), dyn_fma=(44928, 65096), n=N_GUARD, nulls=NULLS_GUARD),
    _c("f-i16-57x57", "features", I16, 57, 57, "wide_supported: first square layout refused",
       (BA, PACKED, FFE), (45760, 42872, 1088), n=10),
    _c("f-i16-33x33", "features", I16, 33, 33, "guard follow-up: C > 16, a second grid trip",
       (BA, WW), (46480, 38152), dyn_fma=(46480, 38416), n=N_GUARD, nulls=NULLS_GUARD),
    _c("f-i16-32x31", "features", I16, 32, 31, "compile-time frame size at its widest C",
       (BA, WW), (51456, 36872), dyn_fma=(51456, 37120), n=18),
    _c("f-i16-32x32", "features", I16, 32, 32, "the 32-of-32 montage's own kernel",
       (BA, C32K), (51456, None), n=18),
    _c("f-i16-3x3", "features", I16, 3, 3, "the 3-of-3 layout's own kernels",
       ("baseline_kernel", "window_kernel"), (None, None), n=24),
    _c("f-i16-32x31-off8", "features", I16, 32, 31, "out 8 off: same kernels, 8-byte stores",
       (BA, WW), (51456, 36872), dyn_fma=(51456, 37120), n=18, shifted=True),
    _c("f-i16-32x32-off8", "features", I16, 32, 32, "out 8 off: 32-of-32 to the generic kernel, "
       "compile-time frame size", (BA, WW), (51456, 37000), dyn_fma=(51456, 37256), n=18,
       shifted=True),
    _c("f-i16-3x3-off8", "features", I16, 3, 3, "out 8 off: 3-of-3 to the generic kernels",
       (BA, WW), (54400, 7184), dyn_fma=(54400, 7232), n=24, shifted=True),
    _c("f-f32-15x3", "features", F32, 15, 3, "two: last float32 layout at two epochs",
       (BA, WW), (54288, 62480), dyn_fma=(54288, 62528), n=20),
    _c("f-f32-16x3", "features", F32, 16, 3, "two: first float32 layout at one epoch",
       (BA, WW), (51456, 33288), dyn_fma=(51456, 33312), n=18),
    _c("f-f32-31x3", "features", F32, 31, 3, "wide_supported: last float32 ct at C = 3",
       (BA, WW), (49728, 64008), dyn_fma=(49728, 64032), n=10),
    _c("f-f32-32x3", "features", F32, 32, 3, "wide_supported: first float32 refused",
       (BA, SMALLW, FFE), (51328, None, 3136), n=10),
    _c("f-f32-29x29", "features", F32, 29, 29, "wide_supported: last square float32 layout",
       (BA, WW), (46528, 63240), dyn_fma=(46528, 63472), n=10),
    _c("f-f32-30x30", "features", F32, 30, 30, "wide_supported: first square float32 refused",
       (BA, LDS, FFE), (48128, 46624, 1088), n=10),
    # ---- process_recording_epochs: the one pass ---------------------------------------------------
    _c("o-i16-40x5", "one_pass", I16, 40, 5, "one pass: whole-dword frames, last before 41",
       (BA, LDS), (56224, 63536), n=16),
    _c("o-i16-41x5", "one_pass", I16, 41, 5, "one pass: packed frames",
       (BA, PACKED), (49440, 62048), n=14),
    _c("o-i16-42x5", "one_pass", I16, 42, 5, "cut_features_fit: refused, 88-byte padded frames",
       (BA, DIRECT, FFE), (50592, None, 5184), n=14),
    _c("o-i16-43x5", "one_pass", I16, 43, 5, "cut_features_fit: last int16 layout, packed",
       (BA, PACKED), (51840, 65040), n=14),
    _c("o-i16-44x6", "one_pass", I16, 44, 6, "cut_features_fit: first refused past 43",
       (BA, LDS, FFE), (52992, 34592, 6208), n=14),
    _c("o-i16-43x43", "one_pass", I16, 43, 43, "cut_features_fit: last layout, two channel passes",
       (BA, PACKED), (43200, 65040), n=12),
    _c("o-f32-20x5", "one_pass", F32, 20, 5, "cut_features_fit: last float32 layout",
       (BA, LDS), (56224, 63536), n=16),
    _c("o-f32-21x5", "one_pass", F32, 21, 5, "cut_features_fit: first float32 refused",
       (BA, DIRECT, FFE), (50592, None, 5184), n=14),
    _c("o-f32-20x20", "one_pass", F32, 20, 20, "cut_features_fit: last float32, every channel",
       (BA, LDS), (56224, 63536), n=16),
    # ---- cut_epochs: chunks, stage, small ---------------------------------------------------------
    _c("c-i16-40x5", "cut", I16, 40, 5, "chunks: last int16 dword layout in one chunk",
       (BA, LDS), (56224, 63000), n=16),
    _c("c-i16-42x6", "cut", I16, 42, 6, "chunks: first dword layout in two",
       (BA, LDS), (50592, 33088), n=14),
    _c("c-i16-43x6", "cut", I16, 43, 6, "chunks: last packed layout in one chunk",
       (BA, PACKED), (51840, 64508), n=14),
    _c("c-i16-45x6", "cut", I16, 45, 6, "chunks: first packed layout in two",
       (BA, PACKED), (54240, 33848), n=14),
    _c("c-i16-86x11", "cut", I16, 86, 11, "chunks: dword frames beside the packed edge",
       (BA, LDS), (51696, 44000), n=8),
    _c("c-i16-87x11", "cut", I16, 87, 11, "chunks: last packed layout in two, 65,432 B",
       (BA, PACKED), (52320, 65432), n=8),
    _c("c-i16-88x11", "cut", I16, 88, 11, "chunks: dword frames in three",
       (BA, LDS), (52896, 45000), n=8),
    _c("c-i16-89x12", "cut", I16, 89, 12, "chunks: first packed layout in three",
       (BA, PACKED), (53520, 44508), n=8),
    _c("c-i16-128x16", "cut", I16, 128, 16, "chunks: last dword layout in three, 65,000 B; "
       "the stage rule's equality", (BA, LDS), (51264, 65000), n=6),
    _c("c-i16-129x17", "cut", I16, 129, 17, "chunks: packed frames in three beside the edge",
       (BA, PACKED), (51680, 64508), n=6),
    _c("c-i16-130x17", "cut", I16, 130, 17, "chunks: first dword layout in four",
       (BA, LDS), (52064, 49632), n=6),
    _c("c-i16-172x22", "cut", I16, 172, 22, "chunks: four dword chunks of 65,424 B, the closest "
       "cut_write_lds_kernel comes to its limit", (BA, LDS), (34432, 65424), n=4),
    _c("c-f32-20x5", "cut", F32, 20, 5, "chunks: last float32 layout in one chunk",
       (BA, LDS), (56224, 63000), n=16),
    _c("c-f32-21x6", "cut", F32, 21, 6, "chunks: first float32 layout in two",
       (BA, LDS), (50592, 33088), n=14),
    _c("c-f32-42x11", "cut", F32, 42, 11, "chunks: last float32 layout in two",
       (BA, LDS), (50496, 64672), n=8),
    _c("c-f32-43x11", "cut", F32, 43, 11, "chunks: first float32 layout in three",
       (BA, LDS), (51696, 44000), n=8),
    _c("c-i16-24x3", "cut", I16, 24, 3, "stage: last int16 ct staged at C = 3",
       (BA, LDS), (53152, 39000), n=24),
    _c("c-i16-25x3", "cut", I16, 25, 3, "stage: first ct read directly at C = 3",
       (BA, SMALLW), (55440, None), n=24),
    _c("c-i16-25x4", "cut", I16, 25, 4, "stage: one more channel stages ct = 25 again",
       (BA, PACKED), (55440, 37508), n=24),
    _c("c-f32-12x3", "cut", F32, 12, 3, "stage: last float32 ct staged at C = 3",
       (BA, LDS), (53152, 39000), n=24),
    _c("c-f32-13x3", "cut", F32, 13, 3, "stage: first float32 ct read directly",
       (BA, SMALLW), (52320, None), n=22),
    _c("c-i16-33x3", "cut", I16, 33, 3, "small: last C of the pairs-in-registers writer",
       (BA, SMALLW), (53120, None), n=18),
    _c("c-i16-33x4", "cut", I16, 33, 4, "small: first C of the direct writer",
       (BA, DIRECT), (53120, None), n=18),
    # ---- the baseline tile, through cut_epochs and process_recording ------------------------------
    _c("c-i16-327x2", "cut", I16, 327, 2, "baseline_any_supported: last int16 ct, 65,440 B",
       (BA, SMALLW), (65440, None), n=4),
    _c("c-i16-328x2", "cut", I16, 328, 2, "baseline_any_supported: first refused",
       (FALLBACK,), (None,), n=4),
    _c("f-i16-327x2", "features", I16, 327, 2, "baseline_any_supported: last int16 ct",
       (BA, SMALLW, FFE), (65440, None, 2112), n=4),
    _c("f-i16-328x2", "features", I16, 328, 2, "baseline_any_supported: first refused",
       (FALLBACK, FFE), (None, 2112), n=4),
    _c("c-f32-163x2", "cut", F32, 163, 2, "baseline_any_supported: last float32 ct",
       (BA, SMALLW), (65232, None), n=4),
    _c("c-f32-164x2", "cut", F32, 164, 2, "baseline_any_supported: first float32 refused",
       (FALLBACK,), (None,), n=4),
    _c("f-f32-163x2", "features", F32, 163, 2, "baseline_any_supported: last float32 ct",
       (BA, SMALLW, FFE), (65232, None, 2112), n=4),
    _c("f-f32-164x2", "features", F32, 164, 2, "baseline_any_supported: first float32 refused",
       (FALLBACK, FFE), (None, 2112), n=4),
    _c("c-i16-64x64", "cut", I16, 64, 64, "baseline_any_tile: four epochs, all 256 lanes",
       (BA, LDS), (51328, 49632), n=10),
    _c("f-i16-64x64", "features", I16, 64, 64, "baseline_any_tile: four epochs, all 256 lanes",
       (BA, LDS, FFE), (51328, 49632, 1088), n=10),
    _c("c-i16-71x64", "cut", I16, 71, 64, "baseline_any_tile: last ct at four epochs",
       (BA, PACKED), (56960, 53400), n=10),
    _c("c-i16-72x64", "cut", I16, 72, 64, "baseline_any_tile: first three-epoch tile",
       (BA, LDS), (43296, 55648), n=8),
    _c("f-i16-72x64", "features", I16, 72, 64, "baseline_any_tile: first three-epoch tile",
       (BA, LDS, FFE), (43296, 55648, 1088), n=8),
    # ---- the batch extract from device epochs -----------------------------------------------------
    _c("x-8x41", "extract", None, 0, 41, "rows_out: last C with the rows in LDS at 8 features",
       (FFE,), (21056,), n=18, nfeat=8),
    _c("x-8x42", "extract", None, 0, 42, "rows_out: first C through `out` at 8 features",
       (FFE,), (1088,), n=18, nfeat=8),
    _c("x-12x27", "extract", None, 0, 27, "rows_out: last C in LDS at 12 features",
       (FFE,), (20800,), n=18, nfeat=12),
    _c("x-12x28", "extract", None, 0, 28, "rows_out: first C through `out` at 12 features",
       (FFE,), (1088,), n=18, nfeat=12),
    _c("x-1x64", "extract", None, 0, 64, "one feature a channel at the widest C",
       (FFE,), (4160,), n=18, nfeat=1),
    # ---- small host batches -----------------------------------------------------------------------
    _c("s-16-n1", "small", None, 0, 16, "features_small_supported: last C, one epoch",
       (FSMALL,), (None,), n=1),
    _c("s-16-n4", "small", None, 0, 16, "features_small_supported: last C, four epochs",
       (FSMALL,), (None,), n=4),
    _c("s-17-n1", "small", None, 0, 17, "features_small_supported: first C round the per-epoch "
       "kernel", (FFE,), (17472,), n=1),
    _c("s-17-n4", "small", None, 0, 17, "features_small_supported: first C refused, four epochs",
       (FFE,), (17472,), n=4),
]
BY_NAME = {c.name: c for c in CASES}

# (last layout of a bucket, first of the next, the predicate that flips between them)
EDGES = [
    ("f-i16-31x3", "f-i16-32x3", "two"), ("f-f32-15x3", "f-f32-16x3", "two"),
    ("f-i16-63x3", "f-i16-64x3", "wide_supported"), ("f-i16-59x32", "f-i16-60x32", "wide_supported"),
    ("f-i16-56x56", "f-i16-57x57", "wide_supported"), ("f-f32-31x3", "f-f32-32x3", "wide_supported"),
    ("f-f32-29x29", "f-f32-30x30", "wide_supported"),
    ("f-i16-32x32", "f-i16-32x32-off8", "out_aligned"), ("f-i16-3x3", "f-i16-3x3-off8", "out_aligned"),
    ("f-i16-32x31", "f-i16-32x32", "c32"),
    ("o-i16-40x5", "o-i16-41x5", "dword_frames"), ("o-i16-41x5", "o-i16-42x5", "one_pass"),
    ("o-i16-42x5", "o-i16-43x5", "one_pass"), ("o-i16-43x5", "o-i16-44x6", "one_pass"),
    ("o-f32-20x5", "o-f32-21x5", "one_pass"),
    ("c-i16-40x5", "c-i16-42x6", "chunks"), ("c-i16-43x6", "c-i16-45x6", "chunks"),
    ("c-i16-87x11", "c-i16-89x12", "chunks"), ("c-i16-86x11", "c-i16-87x11", "chunks"),
    ("c-i16-87x11", "c-i16-88x11", "chunks"),
    ("c-i16-128x16", "c-i16-130x17", "chunks"), ("c-f32-20x5", "c-f32-21x6", "chunks"),
    ("c-f32-42x11", "c-f32-43x11", "chunks"),
    ("c-i16-24x3", "c-i16-25x3", "stage"), ("c-i16-25x3", "c-i16-25x4", "stage"),
    ("c-f32-12x3", "c-f32-13x3", "stage"), ("c-i16-33x3", "c-i16-33x4", "small"),
    ("c-i16-327x2", "c-i16-328x2", "any_supported"), ("f-i16-327x2", "f-i16-328x2", "any_supported"),
    ("c-f32-163x2", "c-f32-164x2", "any_supported"), ("f-f32-163x2", "f-f32-164x2", "any_supported"),
    ("c-i16-71x64", "c-i16-72x64", "any_tile"),
    ("x-8x41", "x-8x42", "rows_out"), ("x-12x27", "x-12x28", "rows_out"),
    ("s-16-n1", "s-17-n1", "small_supported"), ("s-16-n4", "s-17-n4", "small_supported"),
]


def predicate(name, case):
    """The value of a dispatch predicate at a case's layout."""
    fmt = R.fmt_of(case.dtype) if case.dtype else None
    ct, C = case.ct, case.C
    fb = frame_bytes(fmt, ct) if case.dtype else 0
    if name == "chunks":
        packed = fb % 4 != 0
        return cut_chunk_frames(fb if packed else (fb // 4 + 1) * 4, 8 if packed else 0)[1]
    return {
        "two": lambda: wide_two(fmt, ct, C),
        "wide_supported": lambda: R.wide_supported(fmt, ct, C),
        "out_aligned": lambda: not case.shifted,
        "c32": lambda: fmt == INT16 and ct == 32 and C == 32,
        "dword_frames": lambda: fb % 4 == 0,
        "one_pass": lambda: one_pass_writer(fmt, ct, C) is not None,
        "stage": lambda: stage_rule(fmt, ct, C),
        "small": lambda: small_rule(C),
        "any_supported": lambda: R.baseline_any_supported(fmt, ct, C),
        "any_tile": lambda: baseline_any_tile(fmt, ct, C)[0],
        "rows_out": lambda: rows_out(C, case.nfeat),
        "small_supported": lambda: features_small_supported(C),
    }[name]()


# ---- inputs ---------------------------------------------------------------------------------------
N_FRAMES = R.N_FRAMES              # 5,000
SPACING = R.SPACING                # 31: both parities, every 16-byte phase
RESOLUTIONS = [0.1, 0.5, 0.0488281, 1.0, 2.5]
SPARSE_SPACING, SPARSE_N = 805, 6  # n_frames / n = 833 >= 787: the non-temporal variants
STREAM_MIN_SPACING = PRE + 687     # wide.hip launch_baseline_any (the window variants: kWin + 8)
TAIL = 450                         # samples of the last epoch past the recording's end


def selection(case):
    """The last C - 1 columns in reversed order, then column 0: the highest byte offset inside a
    frame is in play, and so is the lowest."""
    cols = list(range(case.ct - 1, case.ct - case.C, -1)) + [0]
    assert len(cols) == case.C and len(set(cols)) == case.C
    return cols, [RESOLUTIONS[i % len(RESOLUTIONS)] for i in range(case.C)]


def null_frames(case):
    """Frames of the alternating stretch the recording starts with: `nulls` whole epochs lie in
    it (900 for the four of refusal_cases.NULL_FRAMES)."""
    return PRE + SPACING * (case.nulls - 1) + 175 + WIN + 20


def recording(dtype, ct, nullf):
    """A random walk (int16) or normal samples (float32) after an alternating stretch."""
    rng = np.random.default_rng(3000 + ct)
    sign = np.where(np.arange(nullf) % 2 == 0, 1.0, -1.0)[:, None]
    if np.dtype(dtype) == np.int16:
        walk = -2000 + np.cumsum(25.0 * rng.standard_normal((N_FRAMES, ct)), axis=0)
        raw = np.clip(np.rint(walk + 40.0 * rng.standard_normal((N_FRAMES, ct))), -32768, 32767)
        raw[:nullf] = 300.0 * sign
    else:
        raw = 50.0 * rng.standard_normal((N_FRAMES, ct))
        raw[:nullf] = 92.5 * sign
    return raw.astype(dtype)


def positions(case):
    """100 + 31 i, and the last epoch's 750 samples run 450 past the end of the recording."""
    pos = PRE + SPACING * np.arange(case.n, dtype=np.int64)
    pos[-1] = N_FRAMES - (POST - TAIL)
    assert case.n < 2 or pos[-2] + POST <= N_FRAMES
    return pos


def sparse_positions():
    pos = PRE + SPARSE_SPACING * np.arange(SPARSE_N, dtype=np.int64)
    assert pos[-1] + POST <= N_FRAMES and N_FRAMES // SPARSE_N >= STREAM_MIN_SPACING
    return pos


def n_nulls(case):
    """Dense rows in the null space: `nulls`, less the last epoch where n is that small."""
    return min(case.nulls, case.n - 1)


def null_rows(case, pos):
    return np.nonzero(pos + 175 + WIN <= null_frames(case))[0]


def epochs_input(case):
    """Device or host epochs [n][C][750] of the extract cases: normal samples, and `nulls` leading
    epochs alternating in every channel (the filters' null space)."""
    rng = np.random.default_rng(4000 + 64 * case.C + case.n)
    ep = 40.0 * rng.standard_normal((case.n, case.C, POST))
    k = min(case.nulls, case.n - 1) if case.n > 1 else 0
    ep[:k] = 92.5 * np.where(np.arange(POST) % 2 == 0, 1.0, -1.0)
    return np.ascontiguousarray(ep), np.arange(k)
