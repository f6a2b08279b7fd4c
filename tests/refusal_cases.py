"""Where the device-side refusals are tested: the library refuses a
marker position the reference would not cut, a label other than 0.0 / 1.0, a non-finite training
feature, a gather index outside its source and an unparsable marker description on the device, and
each of those checks sits in a kernel with a tile, a capped grid or an unrolled loop.  This module
restates those launch constants and dispatch rules, citing where they live, and names the rows and
layouts at which the offending value meets every tile position, trip and unroll slot.  Not a test
module: tests/test_refusal_cases.py pins the restatements to the sources and asserts that every
placement is what its name says; tests/test_gpu_refused_positions.py, tests/test_gpu_refused_rows.py
and tests/test_gpu_plan.py run the device at exactly these placements.
"""
import ast
import os
from collections import namedtuple

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "eeg_dataanalysispackage_amd", "csrc")

INT16, FLOAT32 = 0, 1              # eegfx.h EEGFX_INT_16, EEGFX_IEEE_FLOAT_32
PRE, POST = 100, 750               # dwt8.h kPre, kPost
MAX_CHANNELS = 64                  # launch.h kMaxChannels

# ---- the checkers of a marker position ------------------------------------------------------------
BASELINE_TILE = 64                 # fused.hip launch_fused_baseline: kTile epochs a workgroup
ANY_LANES = 256                    # wide.hip baseline_any_tile: EB = 256 / C
ANY_LDS_TARGET = 56 * 1024         # ... lowered while EB staged runs exceed 56 KB
ANY_LDS_MAX = 64 * 1024            # wide.hip baseline_any_supported
WIDE_LDS_MAX = 64 * 1024           # wide.hip wide_supported
CUT_PAIRS = 5                      # cut.hip kCutPairs: cut_write_small_kernel's pairs a thread
CF_EPOCHS = 8                      # cut.hip kCfEpochs: epochs a workgroup of the c3 kernel
CUT_LDS_MAX = 64 * 1024            # cut.hip EEGFX_CUT_LDS_MAX

# ---- the capped grid-stride loops -----------------------------------------------------------------
THREADS = 256
LR_BLOCKS = 4096                   # logreg.hip launch_lr_validate
CONFUSION_BLOCKS, CONFUSION_UNROLL = 2048, 4     # flow.hip launch_confusion, confusion_kernel's U
GATHER_BLOCKS, GATHER_UNROLL = 2048, 4           # launch.h kGatherMaxBlocks, kGatherUnroll
PLAN_BLOCKS = 8192                 # plan.hip grid_for
BIN_BLOCKS, BIN_PER_THREAD = 8192, 8             # dtree.hip launch_dt_bin: grid_for(n d, 256 * 8, 8192)

LR_TRIP = LR_BLOCKS * THREADS                                    # 1,048,576 rows
CONFUSION_TRIP = CONFUSION_BLOCKS * THREADS * CONFUSION_UNROLL   # 2,097,152 rows
GATHER_TRIP = GATHER_BLOCKS * THREADS * GATHER_UNROLL            # 2,097,152 pieces
PLAN_TRIP = PLAN_BLOCKS * THREADS                                # 2,097,152 markers


def frame_bytes(fmt, ct):
    return ct * (2 if fmt == INT16 else 4)


def baseline_any_tile(fmt, ct, C):
    """wide.hip baseline_any_tile: (EB epochs a workgroup, staged quads an epoch)."""
    bstq = (PRE * frame_bytes(fmt, ct) + 15) // 16 + 2
    eb = ANY_LANES // C
    while eb > 1 and eb * bstq * 16 > ANY_LDS_TARGET:
        eb -= 1
    return eb, bstq


def baseline_any_supported(fmt, ct, C):
    if not 1 <= C <= 256 or ct < 1:
        return False
    eb, bstq = baseline_any_tile(fmt, ct, C)
    return eb * bstq * 16 <= ANY_LDS_MAX


def wide_lds_per_epoch(fmt, ct, C):
    return 8 * (4 * frame_bytes(fmt, ct) + 1) * 16 + 16 * C * 8 + 8 + C * 8


def wide_supported(fmt, ct, C):
    return 1 <= C <= MAX_CHANNELS and ct >= 1 and wide_lds_per_epoch(fmt, ct, C) <= WIDE_LDS_MAX


def is_c3(fmt, ct, C):
    return fmt == INT16 and ct == 3 and C == 3


def checker(fmt, ct, C):
    """(kernel, tile) that raises the error word for a layout the staged baselines take."""
    if is_c3(fmt, ct, C):
        return "baseline_kernel", BASELINE_TILE
    if baseline_any_supported(fmt, ct, C):
        return "baseline_any_kernel", baseline_any_tile(fmt, ct, C)[0]
    return None


def features_route(fmt, ct, C):
    """routes.cpp run_features_from_raw with a 16-byte aligned `out`: (checker, tile, the kernel
    that reads the positions a second time)."""
    if is_c3(fmt, ct, C):   # fused.hip fused_supported; window_kernel reads baseline_kernel's words
        return "baseline_kernel", BASELINE_TILE, "window_kernel"
    if wide_supported(fmt, ct, C):
        eb = baseline_any_tile(fmt, ct, C)[0]
        c32 = fmt == INT16 and ct == 32 and C == 32      # wide.hip launch_window_wide_kernels
        return "baseline_any_kernel", eb, "window_c32_kernel" if c32 else "window_wide_kernel"
    return cut_writer(fmt, ct, C)


def cut_writer(fmt, ct, C, out_aligned=True):
    """cut.hip cut_epochs_impl for a dword-aligned recording: (checker, tile, writer).
    out_aligned: float epochs always; double epochs when `out` lies on a 16-byte boundary."""
    chk = checker(fmt, ct, C) if out_aligned else None
    if chk is None:
        return "cut_epochs_kernel", 1, "cut_epochs_kernel"
    if is_c3(fmt, ct, C):
        return chk + ("cut_features_c3_kernel",)
    fb = frame_bytes(fmt, ct)
    stage = POST * fb <= 2 * 6000 * C
    small = C * (POST // 2) <= THREADS * CUT_PAIRS
    if stage and fb % 4 != 0:
        return chk + ("cut_write_lds_packed_kernel",)
    if stage:
        return chk + ("cut_write_lds_kernel",)
    return chk + ("cut_write_small_kernel" if small else "cut_write_kernel",)


def staged_features_lds(stage_bytes, C):
    return ((max(stage_bytes, (16 * C + 768) * 8) + 15) & ~15) + 64 * 8 + 16


def one_pass_writer(fmt, ct, C):
    """cut.hip cut_features_fit / cut_features_impl for aligned buffers: (checker, tile,
    writer) of the one-pass epochs + features, None where the entry cuts and then extracts."""
    fb = frame_bytes(fmt, ct)
    if not 1 <= C <= MAX_CHANNELS or (fb % 4 != 0 and fmt != INT16) or checker(fmt, ct, C) is None:
        return None
    stage = POST * fb + 8 if fb % 4 != 0 else POST * ((fb // 4 + 1) * 4)
    if staged_features_lds(stage, C) > 64 * 1024:
        return None
    if is_c3(fmt, ct, C):
        return checker(fmt, ct, C) + ("cut_features_c3_kernel",)
    return checker(fmt, ct, C) + ("cut_write_lds_packed_kernel" if fb % 4 != 0
                                  else "cut_write_lds_kernel",)


# The nine kernels that cut "an invalid position as pos = 100", by the file that holds each, and
# the two checkers, which clamp as well.  cut.hip's six kernels call its one cut_position();
# the others carry a copy of the expression each.
CLAMPS = {
    "cut_epochs_kernel": "cut.hip", "cut_write_kernel": "cut.hip",
    "cut_write_small_kernel": "cut.hip", "cut_features_c3_kernel": "cut.hip",
    "cut_write_lds_kernel": "cut.hip", "cut_write_lds_packed_kernel": "cut.hip",
    "window_wide_kernel": "wide.hip", "window_c32_kernel": "wide.hip",
    "exact_rows_kernel": "guard.hip",
}
# the clamps a file holds: cut.hip's are calls of cut_position(), the others copies
CLAMPS_PER_FILE = {"cut.hip": 6, "wide.hip": 3, "guard.hip": 1, "fused.hip": 1}


# ---- layouts --------------------------------------------------------------------------------------
def _tables(module, names):
    """The layout tables of a GPU test module, read without importing it (it needs a device)."""
    tree = ast.parse(open(os.path.join(TESTS, module + ".py")).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) in names:
            out.update(eval(compile(ast.Expression(node.value), module, "eval"), {"np": np}))
    return out


Layout = namedtuple("Layout", "dtype ct cols res")


def layouts():
    """name -> Layout: test_gpu_epochs_f32's LAYOUTS and MORE as "f32/...", test_gpu_pyramid's
    LAYOUTS as "pyramid/...", and the montage neither holds: every one of 32 int16 channels."""
    out = {}
    for name, row in _tables("test_gpu_epochs_f32", ("LAYOUTS", "MORE")).items():
        C = row[4] if len(row) == 5 else len(row[2])
        out["f32/" + name] = Layout(row[0], row[1], list(row[2][:C]), list(row[3][:C]))
    for name, row in _tables("test_gpu_pyramid", ("LAYOUTS",)).items():
        out["pyramid/" + name] = Layout(row[0], row[1], list(row[2]), list(row[3]))
    out["int16_32_of_32"] = Layout(np.int16, 32, list(range(32)), [0.1] * 32)
    return out


def fmt_of(dtype):
    return INT16 if np.dtype(dtype) == np.int16 else FLOAT32


# entry: "features" process_recording, "features64" the same at feature_size = 64 (epochs
# materialised as float32, then the pyramid), "one_pass" process_recording_epochs, "cut" cut_epochs.
# C: the first C selected channels.  epochs: the element types the epochs are asked in.
# shifted: a double `out` 8 bytes off a 16-byte boundary.  kernels: (checker, tile, second reader).
Route = namedtuple("Route", "name entry layout C epochs numerics shifted kernels",
                   defaults=(False, None))
BOTH, EXACT = ("exact", "fma"), ("exact",)
F64_F32 = ("float64", "float32")
ROUTES = [
    Route("features-c3", "features", "pyramid/int16_3", 3, (), BOTH,
          kernels=("baseline_kernel", 64, "window_kernel")),
    Route("features-c32", "features", "int16_32_of_32", 32, (), BOTH,
          kernels=("baseline_any_kernel", 8, "window_c32_kernel")),
    Route("features-wide-int16", "features", "pyramid/int16_5", 3, (), BOTH,
          kernels=("baseline_any_kernel", 55, "window_wide_kernel")),
    Route("features-wide-float32", "features", "pyramid/float32_4", 2, (), BOTH,
          kernels=("baseline_any_kernel", 35, "window_wide_kernel")),
    Route("one-pass-c3", "one_pass", "f32/int16_3", 3, F64_F32, EXACT,
          kernels=("baseline_kernel", 64, "cut_features_c3_kernel")),
    Route("one-pass-packed", "one_pass", "f32/int16_7", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 39, "cut_write_lds_packed_kernel")),
    Route("one-pass-lds-float32", "one_pass", "f32/float32_7", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 20, "cut_write_lds_kernel")),
    Route("one-pass-lds-int16", "one_pass", "f32/int16_32", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 8, "cut_write_lds_kernel")),
    Route("cut-c3", "cut", "f32/int16_3", 3, F64_F32, EXACT,
          kernels=("baseline_kernel", 64, "cut_features_c3_kernel")),
    Route("cut-packed", "cut", "f32/int16_7", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 39, "cut_write_lds_packed_kernel")),
    Route("cut-lds", "cut", "f32/float32_7", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 20, "cut_write_lds_kernel")),
    Route("cut-small", "cut", "f32/int16_70_direct", 3, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 4, "cut_write_small_kernel")),
    Route("cut-direct", "cut", "f32/int16_70_direct", 5, F64_F32, EXACT,
          kernels=("baseline_any_kernel", 4, "cut_write_kernel")),
    Route("cut-fallback-layout", "cut", "f32/int16_400", 2, F64_F32, EXACT,
          kernels=("cut_epochs_kernel", 1, "cut_epochs_kernel")),
    Route("cut-fallback-shifted", "cut", "f32/int16_3", 3, ("float64",), EXACT, shifted=True,
          kernels=("cut_epochs_kernel", 1, "cut_epochs_kernel")),
    Route("features64-packed", "features64", "pyramid/int16_5", 3, (), EXACT,
          kernels=("baseline_any_kernel", 55, "cut_write_lds_packed_kernel")),
]


def restated_kernels(route):
    """What the restated dispatch gives for a route (compared with route.kernels by the CPU test)."""
    lay = layouts()[route.layout]
    fmt = fmt_of(lay.dtype)
    if route.entry == "features":
        return features_route(fmt, lay.ct, route.C)
    if route.entry == "one_pass":
        return one_pass_writer(fmt, lay.ct, route.C)
    return cut_writer(fmt, lay.ct, route.C, out_aligned=not route.shifted)


# ---- placements of a bad position -----------------------------------------------------------------
BAD_POSITION = 99
# test_gpu_robustness.BAD (the overflow-sized values included); n_frames + 101 is added by the test
BAD_VALUES = [99, 0, -1, -(10 ** 15), 10 ** 15, 2 ** 62, -(2 ** 63), 2 ** 63 - 1]
N_FRAMES = 5000
SPACING = 31           # frames between cuts: both parities, every 16-byte phase
NULL_FRAMES = 900      # the recordings start with an alternating stretch: the rows cut at
#                        positions 100, 131, 162 and 193, and every invalid position's (cut as
#                        pos = 100), lie in the filters' null space and fail the fma guard


def epochs_of(tile):
    return 2 * tile + 2


def placements(tile):
    """Indices of the one bad position among 2 T + 2: the first and the last epoch of the first
    tile, the first of the second tile, and the last of the ragged third tile (two epochs)."""
    n = epochs_of(tile)
    return sorted({0, tile - 1, tile, n - 1})


def good_positions(n):
    pos = PRE + SPACING * np.arange(n, dtype=np.int64)
    assert pos[-1] + 175 + 512 <= N_FRAMES
    return pos


def null_space_rows(pos):
    """Valid epochs whose baseline run and window lie wholly in the alternating stretch."""
    return np.nonzero(pos + 175 + 512 <= NULL_FRAMES)[0]


# ---- rows of the capped grid-stride kernels -------------------------------------------------------
def blocks(total, per_block, cap):
    """launch.h grid_for (and its local copies in plan.hip and logreg.hip)."""
    return max(1, min(cap, -(-total // per_block)))


Place = namedtuple("Place", "trip slot block thread")


def place(e, total, per_block, cap, unroll=1):
    """Where element e of `total` runs in a grid-stride loop of blocks(total, per_block, cap)
    workgroups of 256 threads whose trips take `unroll` elements a thread, a grid stride apart."""
    step = blocks(total, per_block, cap) * THREADS
    trip, r = divmod(e, step * unroll)
    slot, r = divmod(r, step)
    return Place(trip, slot, r // THREADS, r % THREADS)


def lr_place(row, n):
    return place(row, n, THREADS, LR_BLOCKS)


def confusion_place(row, n):
    return place(row, n, THREADS * CONFUSION_UNROLL, CONFUSION_BLOCKS, CONFUSION_UNROLL)


def gather_pieces(d, aligned=True):
    """flow.hip launch_gather_rows: 16-byte pieces when d is even and the buffers allow it."""
    return d // 2 if d % 2 == 0 and aligned else d


def gather_place(row, m, d):
    dv = gather_pieces(d)
    return place(row * dv, m * dv, THREADS * GATHER_UNROLL, GATHER_BLOCKS, GATHER_UNROLL)


def plan_place(i, n):
    return place(i, n, THREADS, PLAN_BLOCKS)


def bin_place(row, f, n, d):
    return place(row * d + f, n * d, THREADS * BIN_PER_THREAD, BIN_BLOCKS)


BAD_LABELS = (0.5, float("nan"), 2.0, -1.0)

LR_N = LR_TRIP + 300
LR_ROWS = (0, LR_TRIP - 1, LR_TRIP, LR_N - 1)

CONFUSION_SMALL_N = 1000
CONFUSION_SMALL_ROWS = (255, 256, 511, 512, 767, 768, 999)
CONFUSION_BIG_N = CONFUSION_TRIP + 700

GATHER_N_SRC = 50
GATHER_SHAPES = {1: GATHER_TRIP + 1000, 4: GATHER_TRIP // 2 + 500}     # d -> m


def gather_bad_rows(m):
    return m - 400, m - 1


GATHER_EARLY_ROW = 5

PLAN_SMALL_N = 20
PLAN_BIG_N = PLAN_TRIP + 5000
PLAN_CASES = [(PLAN_SMALL_N, (0,)), (PLAN_SMALL_N, (13,)), (PLAN_SMALL_N, (13, 17)),
              (PLAN_BIG_N, (PLAN_BIG_N - 1000, PLAN_BIG_N - 3))]

TREE_N, TREE_D = 203, 5            # 1015 elements: four trips of one workgroup, the last ragged
TREE_SAMPLED_N, TREE_SAMPLED_D = 10050, 3      # test_gpu_dtree.test_sampled_thresholds' n
