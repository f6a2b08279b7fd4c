"""The cases of tests/test_gpu_sharded_sgd.py and their long-double
restatement, computed once per case.  Not a test module.

Rows come from logreg_reference.rows (unit-norm rows with a planted direction), in position order:
shard s of a case holds the rows [offset_s, offset_s + size_s) unless the case scatters them.  The
shard sizes put, in one run or another, a shard of 0 rows, of 1 row, of fewer than 16 rows (less
than one 16-row group of a wave) and of more than 4 G rows (G = ceil(n / 64) workgroups of 4 waves:
a wave's row loop takes a second trip) on the root and off it."""
import functools
from collections import namedtuple

import numpy as np

import logreg_reference as lr

REL = 1e-9          # the bar of test_gpu_logreg_shapes.py on the weights
CONDITIONED = 1e-4  # no convergence test of a run lies closer to flipping (logreg_reference.Run)

SIZES = {2: (1, 400), 3: (300, 0, 13), 5: (0, 1, 7, 400, 92)}
TRAIN_D = (48, 200)  # lr_grad16_kernel and lr_grad_kernel

Case = namedtuple("Case", "sizes d gradient iters fraction parts seed tol",
                  defaults=(100, 1.0, 4, None, 0.001))


def case_id(c):
    s = f"{c.gradient}-k{len(c.sizes)}-n{sum(c.sizes)}-d{c.d}-it{c.iters}"
    s += f"-f{c.fraction}" if c.fraction < 1.0 else ""
    return s + (f"-tol{c.tol}" if c.tol != 0.001 else "")


FULL_CASES = [Case(SIZES[k], d, g) for g in lr.GRADIENTS for k in (2, 3, 5) for d in TRAIN_D]
# a tolerance the run meets long before its last iteration: what every shard launches after that
# must leave the state alone
CONVERGING = [Case(SIZES[5], d, g, tol=0.02) for g in lr.GRADIENTS for d in TRAIN_D]
FEW_ITERATIONS = [Case(SIZES[3], 48, g, iters=it) for g in lr.GRADIENTS for it in (0, 1)]
# positions interleaved between the shards; 40 rows at 0.03: most samples are empty or one row
# (every other shard's share of it empty); 100 and 300 rows: positions on both sides of the
# 32-bit words of the mask in every shard
SCATTER_CASES = [Case((14, 13, 13), 20, "logistic", fraction=0.03),
                 Case((34, 33, 33), 48, "logistic", fraction=0.5),
                 Case((100, 100, 100), 200, "logistic", fraction=0.5)]
# the same with pos == NULL: shard s holds the positions behind those of shard s - 1
CONTIGUOUS_SAMPLED = [Case((1, 40, 59), 48, "logistic", fraction=0.5)]


@functools.lru_cache(maxsize=None)
def rows(c):
    n = sum(c.sizes)
    X, y = lr.rows(n, c.d, 1000 * c.d + n if c.seed is None else c.seed)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def start(c):
    return lr.initial_weights(c.d)  # nonzero


def sample_rows(c):
    """rows_of_iteration for the restatement: spark_sample of the whole list, as the device draws."""
    from eeg_dataanalysispackage_amd import classification as clf
    n = sum(c.sizes)
    return lambda i: clf.spark_sample(n, c.fraction, c.parts, 42 + i).tolist()


@functools.lru_cache(maxsize=None)
def restated(c):
    X, y = rows(c)
    run = lr.sgd_train(X, y, c.iters, 1.0, 0.01, c.tol, initial=start(c), gradient=c.gradient,
                       rows_of_iteration=sample_rows(c) if c.fraction < 1.0 else None)
    w = np.asarray(run.weights, dtype=np.float64)
    w.setflags(write=False)
    return w, run.iterations, run.conv_margin


def interleaved(c):
    """Position lists of a scatter case: position p lies on shard p mod k while that shard has
    room, in increasing order per shard."""
    k, n = len(c.sizes), sum(c.sizes)
    lists = [[] for _ in range(k)]
    s = 0
    for p in range(n):
        while len(lists[s % k]) >= c.sizes[s % k]:
            s += 1
        lists[s % k].append(p)
        s += 1
    return [np.array(v, dtype=np.int64) for v in lists]
