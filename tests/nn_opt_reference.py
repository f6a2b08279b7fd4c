"""The line-search optimisers of train_clf=nn restated in numpy, formula
by formula, in np.longdouble (or any dtype handed in), on tests/nn_reference.py: the contract the
device code is held to.  Nothing here knows how the kernels order sums or share work.

``line_search`` is a function of a score callback, so synthetic phi tables can drive it.  Every
comparison that selects between formulas or ends a search or a training is recorded in a ``trace``
as (tag, relative margin): the tags of TAGS.  The three clamps (0.5 step, 0.1 step, gamma at 0) are
recorded as tags without a margin: both sides of each are the same value where they meet.
"""
import numpy as np

import nn_reference as ref

LD = np.longdouble
ALGORITHMS = ("line_gradient_descent", "conjugate_gradient", "lbfgs")
HISTORY = 4

LINE_TAGS = ("stepmin:return", "stepmin:go", "rescale:yes", "rescale:no", "armijo:accept",
             "armijo:reject", "finite:no", "finite:yes", "first:yes", "first:no", "a0:yes",
             "a0:no", "disc:neg", "disc:nonneg", "b:nonpos", "b:pos", "best:yes", "best:no",
             "lower:yes", "lower:no", "half:clamp", "half:keep", "tenth:clamp", "tenth:keep")
TRAIN_TAGS = ("zero:stop", "zero:go", "eps:stop", "eps:go", "gamma:clip", "gamma:keep",
              "history:full", "history:growing")
TAGS = LINE_TAGS + TRAIN_TAGS
CONTINUOUS = ("half:", "tenth:", "gamma:", "history:")  # tags that carry no margin


def consts(dtype):
    ten = dtype(10)
    return dict(alf=1 / ten ** 4, tolx=1 / ten ** 7, step_max=dtype(100), eps=1 / ten ** 5)


def margin(a, b):
    """|a - b| relative to the larger of the two; inf where either is not finite or both are 0."""
    a, b = np.longdouble(a), np.longdouble(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return float("inf")
    scale = max(abs(a), abs(b))
    return float(abs(a - b) / scale) if scale > 0 else float("inf")


def note(trace, tag, m=float("inf")):
    assert tag in TAGS, tag
    trace.append((tag, m))


def line_search(phi, s0, slope, norm, test, max_ls, trace, rescale=None, dtype=LD):
    """BackTrackLineSearch as the definition writes it.  phi(step) is the score at p - step * dir
    (dir after `rescale(factor)` was called, which happens before the first trial if at all).
    Returns (step, the score held for that step, trials evaluated)."""
    with np.errstate(all="ignore"):  # a division by zero gives the IEEE value, as on the device
        return _line_search(phi, s0, slope, norm, test, max_ls, trace, rescale, dtype)


def _line_search(phi, s0, slope, norm, test, max_ls, trace, rescale, dtype):
    c = consts(dtype)
    s0, slope = dtype(s0), dtype(slope)
    step_min = c["tolx"] / dtype(test)  # inf for test = 0; a NaN test makes no step too small
    big = norm > c["step_max"]
    note(trace, "rescale:yes" if big else "rescale:no", margin(norm, c["step_max"]))
    if big and rescale is not None:
        rescale(c["step_max"] / dtype(norm))
    step, step2 = dtype(1), dtype(0)
    sc = sc2 = best = s0
    best_step = dtype(1)
    trials, lowered = 0, False
    for _ in range(max_ls):
        small = step < step_min
        note(trace, "stepmin:return" if small else "stepmin:go", margin(step, step_min))
        if small:
            return dtype(0), s0, trials
        prev, sc = sc, dtype(phi(step))
        trials += 1
        lower = bool(sc < best)
        note(trace, "lower:yes" if lower else "lower:no", margin(sc, best))
        if lower:
            best, best_step, lowered = sc, step, True
        bound = s0 + c["alf"] * step * slope
        ok = bool(sc <= bound)
        note(trace, "armijo:accept" if ok else "armijo:reject", margin(sc, bound))
        if ok:
            return step, sc, trials
        finite = bool(np.isfinite(sc) and np.isfinite(prev))
        note(trace, "finite:yes" if finite else "finite:no")
        if not finite:
            tmp = step / 5
        elif step == 1:
            note(trace, "first:yes")
            tmp = -slope / (2 * (sc - s0 - slope))
        else:
            note(trace, "first:no", margin(step, 1))
            r1 = sc - s0 - step * slope
            r2 = sc2 - s0 - step2 * slope
            q1, q2 = r1 / (step * step), r2 / (step2 * step2)
            a = (q1 - q2) / (step - step2)
            b = (-step2 * q1 + step * q2) / (step - step2)
            note(trace, "a0:yes" if a == 0 else "a0:no", margin(q1, q2))
            if a == 0:
                tmp = -slope / (2 * b)
            else:
                disc = b * b - 3 * a * slope
                note(trace, "disc:neg" if disc < 0 else "disc:nonneg",
                     margin(b * b, 3 * a * slope))
                if disc < 0:
                    tmp = step / 2
                else:
                    note(trace, "b:nonpos" if b <= 0 else "b:pos", margin(step2 * q1, step * q2))
                    tmp = (-b + np.sqrt(disc)) / (3 * a) if b <= 0 else -slope / (b + np.sqrt(disc))
            keep = bool(tmp < step / 2)
            note(trace, "half:keep" if keep else "half:clamp")
            if not keep:
                tmp = step / 2
        step2, sc2 = step, sc
        keep = bool(tmp > step / 10)
        note(trace, "tenth:keep" if keep else "tenth:clamp")
        step = tmp if keep else step / 10
    won = bool(best < s0)
    # best is s0 itself until a trial lowers it: no margin to take then
    note(trace, "best:yes" if won else "best:no", margin(best, s0) if lowered else float("inf"))
    return (best_step, best, trials) if won else (dtype(0), s0, trials)


def search_constants(p, g, d, dtype=LD):
    """(norm, slope, test) of line_search's head for parameters p, gradient g, direction d."""
    norm = np.sqrt(np.sum(d * d))
    slope = -np.sum(d * g)
    ap = np.abs(p)
    test = np.max(np.abs(g) / np.where(ap > 1, ap, dtype(1)))  # a NaN among them makes it a NaN
    return norm, slope, test


def cg_direction(g, g_new, d, trace):
    """gamma = max(dgg / gg, 0) (a NaN stays); gamma * d + g_new."""
    dgg, gg = np.sum((g_new - g) * g_new), np.sum(g * g)
    q = dgg / gg
    clip = bool(q < 0)
    note(trace, "gamma:clip" if clip else "gamma:keep")
    return (d.dtype.type(0) if clip else q) * d + g_new


def lbfgs_direction(history, s, yv, g_new, trace, dtype=LD):
    """Pushes (s, y, rho) at the front of `history` (a list, newest first), runs the two loops."""
    eps = consts(dtype)["eps"]
    sy, yy = np.sum(s * yv) + eps, np.sum(yv * yv) + eps
    history.insert(0, (s, yv, 1 / sy))
    full = len(history) > HISTORY
    note(trace, "history:full" if full else "history:growing")
    del history[HISTORY:]
    q = g_new.copy()
    alpha = []
    for sk, yk, rho in history:  # newest -> oldest
        a = rho * np.sum(sk * q)
        alpha.append(a)
        q = q - a * yk
    q = q * (sy / yy)
    for (sk, yk, rho), a in zip(history[::-1], alpha[::-1]):  # oldest -> newest
        b = rho * np.sum(yk * q)
        q = q + (a - b) * sk
    return q


def train_opt(params0, X, y, spec, algorithm, iterations, max_ls=5, dtype=LD, reverse=False):
    """The definition's training loop.  Returns dict(params, scores, steps, search_scores, trials,
    iterations_run, trace); scores / steps / ... hold iterations_run entries."""
    assert algorithm in ALGORITHMS
    Xs, ys = (np.asarray(X)[::-1], np.asarray(y)[::-1]) if reverse else (X, y)
    p = np.asarray(params0).astype(dtype)
    state = ref.updater_state(p.size, dtype)
    upd = lambda grad, t: ref.updater_step(spec["updater"], grad, state, spec["learning_rate"],
                                           spec["momentum"], t, dtype)
    trace = []
    with np.errstate(all="ignore"):
        score, grad = ref.loss_and_gradient(p, X, y, spec, dtype, reverse)
        g = upd(grad, 1)
        d = g.copy()
        p_old, g_old, history = p.copy(), g.copy(), []
        out = dict(scores=[], steps=[], search_scores=[], trials=[], iterations_run=0)
        for i in range(iterations):
            out["scores"].append(score)
            norm, slope, test = search_constants(p, g, d, dtype)
            box = [d]

            def rescale(f):
                box[0] = box[0] * f

            phi = lambda step: ref.loss_of(p - step * box[0], Xs, ys, spec, dtype)
            step, held, trials = line_search(phi, score, slope, norm, test, max_ls, trace, rescale,
                                             dtype)
            d = box[0]
            out["steps"].append(step)
            out["search_scores"].append(held)
            out["trials"].append(trials)
            if step != 0:
                p = p - step * d
            old = score
            score, grad = ref.loss_and_gradient(p, X, y, spec, dtype, reverse)
            g_new = upd(grad, i + 2)
            if algorithm == "line_gradient_descent":
                d = g_new.copy()
            elif algorithm == "conjugate_gradient":
                d = cg_direction(g, g_new, d, trace)
            else:
                d = lbfgs_direction(history, p - p_old, g_new - g_old, g_new, trace, dtype)
                p_old, g_old = p.copy(), g_new.copy()
            g = g_new
            out["iterations_run"] = i + 1
            asum = np.sum(np.abs(g))
            note(trace, "zero:stop" if asum == 0 else "zero:go")
            if asum == 0:
                break
            lhs = 2 * abs(old - score)
            rhs = consts(dtype)["eps"] * (abs(old) + abs(score) + 1 / dtype(10) ** 4)
            stop = bool(not (score == 0 and old == 0) and lhs <= rhs)
            note(trace, "eps:stop" if stop else "eps:go", margin(lhs, rhs))
            if stop:
                break
    out["params"] = p
    out["trace"] = trace
    for k in ("scores", "steps", "search_scores"):
        out[k] = np.array(out[k], dtype=dtype)
    out["trials"] = np.array(out["trials"], dtype=np.int64)
    return out


def tags_of(trace):
    return [t for t, _ in trace]


def smallest_margin(trace):
    """(margin, tag) of the closest recorded decision that carries a margin."""
    rows = [(m, t) for t, m in trace if not t.startswith(CONTINUOUS)]
    return min(rows) if rows else (float("inf"), "")
