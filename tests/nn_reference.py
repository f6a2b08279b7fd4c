"""The dense network of train_clf=nn restated in numpy, formula by formula,
in np.longdouble (or any dtype handed in): the contract the device code is held to.  Nothing here
knows how the kernels tile rows or order sums; rows are summed in array order (or reversed).

A model is ``spec = dict(d=, widths=, activations=, loss=, updater=, learning_rate=, momentum=)``
with the names already mapped (unknown strings are the caller's business).  The flat parameter
vector holds, layer after layer, W[n_in][n_out] row-major and then b[n_out].
"""
import numpy as np

LD = np.longdouble


def layer_shapes(d, widths):
    n_in = [d] + list(widths[:-1])
    return list(zip(n_in, widths))


def param_count(d, widths):
    return sum(i * o + o for i, o in layer_shapes(d, widths))


def unpack(params, d, widths, dtype=LD):
    """[(W, b)] of every layer, views of a copy of `params` in `dtype`."""
    p = np.asarray(params).astype(dtype)
    layers, at = [], 0
    for n_in, n_out in layer_shapes(d, widths):
        W = p[at:at + n_in * n_out].reshape(n_in, n_out)
        at += n_in * n_out
        layers.append((W, p[at:at + n_out]))
        at += n_out
    assert at == p.size
    return layers


def sigmoid(z):
    return 1 / (1 + np.exp(-z))


def activate(name, z):
    """f(z), row-wise for softmax (max-subtracted)."""
    if name == "sigmoid":
        return sigmoid(z)
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.maximum(z, 0)  # a NaN stays a NaN
    if name == "identity":
        return z
    if name == "softplus":
        return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))
    if name == "elu":
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    if name == "softmax":
        e = np.exp(z - np.max(z, axis=1, keepdims=True))
        return e / np.sum(e, axis=1, keepdims=True)
    raise ValueError(name)


def activate_prime(name, z):
    """f'(z), elementwise (softmax has a Jacobian instead: backprop_through)."""
    one = np.ones_like(z)
    if name == "sigmoid":
        s = sigmoid(z)
        return s * (1 - s)
    if name == "tanh":
        return 1 - np.tanh(z) ** 2
    if name == "relu":
        return np.where(z > 0, one, 0 * one)
    if name == "identity":
        return one
    if name == "softplus":
        return sigmoid(z)
    if name == "elu":
        return np.where(z > 0, one, np.exp(np.minimum(z, 0)))
    raise ValueError(name)


def backprop_through(name, z, a, upstream):
    """dL/dz from dL/da = upstream."""
    if name == "softmax":  # da_k/dz_m = a_k (delta_km - a_m)
        return a * (upstream - np.sum(upstream * a, axis=1, keepdims=True))
    return upstream * activate_prime(name, z)


def labels_matrix(y, dtype=LD):
    """labels[i] = {t, |1 - t|} (NeuralNetworkClassifier.java:82-83)."""
    t = np.asarray(y).astype(dtype)
    return np.stack([t, np.abs(1 - t)], axis=1)


def row_losses(loss, p, y):
    if loss == "xent":
        return -np.sum(y * np.log(p) + (1 - y) * np.log(1 - p), axis=1)
    if loss == "negativeloglikelihood":
        return -np.sum(y * np.log(p), axis=1)
    if loss == "mse":
        return np.sum((p - y) ** 2, axis=1) / 2
    if loss == "squared_loss":
        return np.sum((p - y) ** 2, axis=1)
    raise ValueError(loss)


def loss_prime(loss, p, y):
    if loss == "xent":
        return -y / p + (1 - y) / (1 - p)
    if loss == "negativeloglikelihood":
        return -y / p
    if loss == "mse":
        return p - y
    if loss == "squared_loss":
        return 2 * (p - y)
    raise ValueError(loss)


def forward(layers, activations, X):
    """[(z, a)] per layer for the rows of X."""
    out, a = [], X
    for (W, b), name in zip(layers, activations):
        z = a @ W + b
        a = activate(name, z)
        out.append((z, a))
    return out


def loss_of(params, X, y, spec, dtype=LD):
    """The mean loss over the rows."""
    layers = unpack(params, spec["d"], spec["widths"], dtype)
    Xd = np.asarray(X).astype(dtype)
    p = forward(layers, spec["activations"], Xd)[-1][1]
    return np.sum(row_losses(spec["loss"], p, labels_matrix(y, dtype))) / dtype(len(Xd))


def loss_and_gradient(params, X, y, spec, dtype=LD, reverse=False):
    """(mean loss, flat gradient of it): every row's terms summed in array order (reverse: from
    the last row to the first), then divided by n."""
    layers = unpack(params, spec["d"], spec["widths"], dtype)
    Xd = np.asarray(X).astype(dtype)
    Y = labels_matrix(y, dtype)
    if reverse:
        Xd, Y = Xd[::-1], Y[::-1]
    acts, loss = spec["activations"], spec["loss"]
    fw = forward(layers, acts, Xd)
    z, p = fw[-1]
    closed = (loss, acts[-1]) in (("xent", "sigmoid"), ("negativeloglikelihood", "softmax"))
    delta = p - Y if closed else backprop_through(acts[-1], z, p, loss_prime(loss, p, Y))
    grads = []
    for l in range(len(layers) - 1, -1, -1):
        a_prev = Xd if l == 0 else fw[l - 1][1]
        dW = np.zeros_like(layers[l][0])
        db = np.zeros_like(layers[l][1])
        for r in range(len(Xd)):  # row after row
            dW += np.outer(a_prev[r], delta[r])
            db += delta[r]
        grads.append((dW, db))
        if l > 0:
            delta = backprop_through(acts[l - 1], fw[l - 1][0], fw[l - 1][1],
                                     delta @ layers[l][0].T)
    n = dtype(len(Xd))
    flat = np.concatenate([np.concatenate([dW.reshape(-1), db]) for dW, db in grads[::-1]]) / n
    total = dtype(0)
    for v in row_losses(loss, p, Y):
        total += v
    return total / n, flat


def updater_state(count, dtype=LD):
    return [np.zeros(count, dtype=dtype), np.zeros(count, dtype=dtype)]


def updater_step(name, g, state, lr, mu, t, dtype=LD):
    """The update u (p <- p - u) of iteration t = 1, 2, ...; `state` is advanced in place."""
    lr, mu = dtype(lr), dtype(mu)
    s1, s2 = state
    if name == "sgd":
        return lr * g
    if name == "nesterovs":
        v = s1.copy()
        s1[:] = mu * v - lr * g
        return mu * v - (1 + mu) * s1
    if name == "adam":
        b1, b2, eps = dtype(9) / 10, dtype(999) / 1000, dtype(1) / 10 ** 8
        s1[:] = b1 * s1 + (1 - b1) * g
        s2[:] = b2 * s2 + (1 - b2) * g * g
        return lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * s1 / (np.sqrt(s2) + eps)
    if name == "adagrad":
        s1[:] = s1 + g * g
        return lr * g / (np.sqrt(s1) + dtype(1) / 10 ** 6)
    if name == "rmsprop":
        s1[:] = dtype(95) / 100 * s1 + dtype(5) / 100 * g * g
        return lr * g / np.sqrt(s1 + dtype(1) / 10 ** 8)
    raise ValueError(name)


def train(params0, X, y, spec, iterations, dtype=LD, reverse=False):
    """(params, scores): `iterations` full-batch steps; scores[i] = the loss before step i."""
    p = np.asarray(params0).astype(dtype)
    state = updater_state(p.size, dtype)
    scores = []
    for t in range(1, iterations + 1):
        loss, g = loss_and_gradient(p, X, y, spec, dtype, reverse)
        scores.append(loss)
        p = p - updater_step(spec["updater"], g, state, spec["learning_rate"], spec["momentum"],
                             t, dtype)
    return p, np.array(scores, dtype=dtype)


def predict(params, X, spec, dtype=LD):
    """Output 0 of the last layer per row."""
    layers = unpack(params, spec["d"], spec["widths"], dtype)
    return forward(layers, spec["activations"], np.asarray(X).astype(dtype))[-1][1][:, 0]
