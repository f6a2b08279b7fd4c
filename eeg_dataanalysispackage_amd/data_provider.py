"""OffLineDataProvider -- the reference's data-provider API on the MI355X path.

Mirrors DataTransformation/OffLineDataProvider.java: ``OffLineDataProvider(args)`` (:78),
``loadData()`` (:88-98), ``getData()`` (:370), ``getDataLabels()`` (:377), with the same argument
formats (``[info.txt]`` or ``[file.eeg, guessed, ...]``), the same per-file skip rules and the
same error behaviour: ``loadData`` never raises -- it logs the fatal error, keeps what was loaded
and exposes the message as ``last_error``.  Paths are local files (the reference reads HDFS).

Decode, epoch cut and baseline correction run on the GPU (csrc/cut.hip); the epochs stay
resident in HBM and ``getData()`` copies them back.

``OffLineDataProvider(args, contexts=[...])`` shards ``loadData()`` over several contexts (any mix
of devices): one host planning pass, then one worker per context on its ``shard_range`` slice of
the selected epochs.  The getters return the same rows in the same order; ``getShards()`` exposes
each shard's resident device buffers (include/eegfx.h, eegfx_odp_create_multi), and
``splitShards()`` the train/test split of their feature rows, kept where the rows are.
"""
from __future__ import annotations

import ctypes
import logging
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, lib
from .context import Context

log = logging.getLogger(__name__)


class _DeviceView:
    """A device array of a shard (``__cuda_array_interface__`` version 2, float64):
    ``torch.as_tensor(view, device="cuda")`` wraps it without a copy.  The memory belongs to the
    provider and is read-only by contract -- nothing may write through the view.  The interface's
    read-only flag stays False all the same: torch refuses an array that sets it ("the read only
    flag is not supported"), and a view nobody can wrap would serve no one.  Valid until the
    provider's next ``loadData()`` or ``close()``; keeps the provider alive."""

    read_only = True

    def __init__(self, owner, address, shape):
        self._owner = owner
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": "<f8",
                                         "data": (int(address or 0), False), "version": 2,
                                         "strides": None}


class Shard:
    """One shard of a provider (eegfx_odp_shard): the epochs ``[first, first + count)`` of
    ``getData()`` order, resident on context ``ctx_index`` (HIP device ``device``, -1 for a
    planning-only provider).  ``epochs`` (count, 3, 750) and ``features`` (count, 48) are device
    views; ``features_numerics`` is EXACT / FMA of those rows, -1 when there are none."""

    def __init__(self, owner, s):
        self.ctx_index, self.device = int(s.ctx_index), int(s.device)
        self.first, self.count = int(s.first), int(s.count)
        self.features_numerics = int(s.features_numerics)
        self.epochs = _DeviceView(owner, s.epochs, (self.count if s.epochs else 0, 3,
                                                    _lib.POSTSTIMULUS))
        self.features = _DeviceView(owner, s.features, (self.count if s.features else 0, 48))

    def __repr__(self):
        return (f"Shard(ctx_index={self.ctx_index}, device={self.device}, first={self.first}, "
                f"count={self.count}, features_numerics={self.features_numerics})")


class _IndexView(_DeviceView):
    """A device array of int64 positions; otherwise a _DeviceView."""

    def __init__(self, owner, address, shape):
        super().__init__(owner, address, shape)
        self.__cuda_array_interface__["typestr"] = "<i8"


def _tensor(view, device):
    """The view as a torch tensor on its device (no copy); an empty tensor for no rows."""
    import torch
    if 0 in view.shape:
        dtype = torch.int64 if isinstance(view, _IndexView) else torch.float64
        return torch.empty(view.shape, dtype=dtype, device=f"cuda:{device}")
    return torch.as_tensor(view, device=f"cuda:{device}")


class SplitShard:
    """One shard's part of the train/test split (eegfx_split_shard), on context ``ctx_index``
    (``context``): ``X_train`` (n_train, d), ``y_train`` (n_train) and ``pos_train`` (n_train,
    int64: the position of each row in the training part of the shuffled list, increasing), and
    the same for the test part.  Torch tensors over the provider's buffers, read-only by
    contract, valid until the provider's next ``splitShards()``, ``loadData()`` or ``close()``."""

    def __init__(self, owner, s, d, context):
        self.ctx_index, self.context = int(s.ctx_index), context
        self.n_train, self.n_test = int(s.n_train), int(s.n_test)
        dev = context.device
        for part, n in (("train", self.n_train), ("test", self.n_test)):
            setattr(self, "X_" + part,
                    _tensor(_DeviceView(owner, getattr(s, "X_" + part), (n, d)), dev))
            setattr(self, "y_" + part,
                    _tensor(_DeviceView(owner, getattr(s, "y_" + part), (n,)), dev))
            setattr(self, "pos_" + part,
                    _tensor(_IndexView(owner, getattr(s, "pos_" + part), (n,)), dev))

    def __repr__(self):
        return (f"SplitShard(ctx_index={self.ctx_index}, n_train={self.n_train}, "
                f"n_test={self.n_test})")


class OffLineDataProvider:
    def __init__(self, args: Sequence[str], context: Optional[Context] = None,
                 plan_only: bool = False, contexts: Optional[Sequence[Context]] = None,
                 shards: Optional[int] = None):
        """plan_only=True: parse, select and label on the host only (no GPU, no epochs).
        contexts=[Context, ...]: a provider over several contexts (eegfx_odp_create_multi), any
        mix of devices; loadData() shards the selected epochs over them (getShards()).
        plan_only=True, shards=k: the planning-only provider that reports the same k ranges."""
        self.args = list(args)
        argv = (ctypes.c_char_p * max(1, len(self.args)))(*[a.encode() for a in self.args])
        h = ctypes.c_void_p()
        if contexts is not None or shards is not None:
            if context is not None:
                raise ValueError("give either context or contexts")
            if plan_only:
                if contexts is not None or shards is None:
                    raise ValueError("a planning-only sharded provider takes shards=k, no contexts")
                self._ctxs, n, handles = [], int(shards), None
            else:
                if contexts is None or (shards is not None and shards != len(contexts)):
                    raise ValueError("shards must equal len(contexts)")
                self._ctxs = list(contexts)
                n = len(self._ctxs)
                handles = (ctypes.c_void_p * max(1, n))(*[c.handle for c in self._ctxs])
            self._ctx = None
            check(lib().eegfx_odp_create_multi(handles, n, argv, len(self.args), ctypes.byref(h)))
        else:
            self._ctx = None if plan_only else (context if context is not None else Context())
            self._ctxs = [] if self._ctx is None else [self._ctx]
            handle = self._ctx.handle if self._ctx is not None else None
            check(lib().eegfx_odp_create(handle, argv, len(self.args), ctypes.byref(h)))
        self._h = h
        self.last_error = ""
        log.info("Started OffLineDataProvider with arguments %s", self.args)

    def getShards(self) -> List[Shard]:
        """The provider's shards in list order (one for a one-context provider)."""
        out = []
        for i in range(int(lib().eegfx_odp_num_shards(self._h))):
            s = _lib.OdpShard()
            check(lib().eegfx_odp_get_shard(self._h, i, ctypes.byref(s)))
            out.append(Shard(self, s))
        return out

    def loadData(self) -> None:
        rc = lib().eegfx_odp_load_data(self._h)
        self.last_error = lib().eegfx_odp_error(self._h).decode(errors="replace")
        if rc != _lib.EEGFX_OK:
            log.critical(self.last_error)  # logger.fatal(e.getMessage()) -- swallowed

    def num_epochs(self) -> int:
        return int(lib().eegfx_odp_num_epochs(self._h))

    def getData(self, dtype=np.float64) -> np.ndarray:
        """Epochs as double[n][3][750] (Fz, Cz, Pz).  dtype=np.float32: the same values as
        float[n][3][750] (eegfx_odp_get_data_f32 -- every epoch sample is a widened fp32, so
        nothing is lost and half the bytes cross the host link)."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError(f"epochs are float64 or float32, got {dtype}")
        n = self.num_epochs()
        out = np.empty((n, 3, _lib.POSTSTIMULUS), dtype=dtype)
        if n:
            fn = lib().eegfx_odp_get_data if dtype == np.float64 else lib().eegfx_odp_get_data_f32
            check(fn(self._h, ctypes.c_void_p(out.ctypes.data)))
        return out

    def getDataLabels(self) -> List[float]:
        n = self.num_epochs()
        out = np.empty(max(1, n), dtype=np.float64)
        check(lib().eegfx_odp_get_labels(self._h, ctypes.c_void_p(out.ctypes.data)))
        return [float(v) for v in out[:n]]

    def getPositions(self):
        """Marker positions and source-file index of every selected epoch (not in the Java API;
        exposes the bit-exact marker offsets for parity tests)."""
        n = self.num_epochs()
        pos = np.empty(max(1, n), dtype=np.int64)
        fid = np.empty(max(1, n), dtype=np.int32)
        check(lib().eegfx_odp_get_positions(self._h, ctypes.c_void_p(pos.ctypes.data),
                                            ctypes.c_void_p(fid.ctypes.data)))
        return pos[:n], fid[:n]

    def getFeatures(self, name=8, epoch_size=512, skip=175, feature_size=16) -> np.ndarray:
        """fe=dwt-8 features of the resident epochs, computed on the device: [n][3*feature_size],
        feature_size <= 512 (the first feature_size coefficients of each channel's pyramid)."""
        n = self.num_epochs()
        out = np.empty((n, 3 * feature_size), dtype=np.float64)
        if n:
            check(lib().eegfx_odp_get_features(self._h, name, epoch_size, skip, feature_size,
                                               ctypes.c_void_p(out.ctypes.data)))
        return out

    def split(self, fe=None, seed: int = 1, train_fraction: float = 0.7, device: bool = True,
              context: Optional[Context] = None):
        """The train/test data of PipelineBuilder.execute (:177-187) without a trip through host
        memory (eegfx_odp_split): the rows of getFeatures(fe's parameters) and the labels, both
        in the order of Collections.shuffle(list, new Random(seed)), cut at
        int(n * train_fraction).  Returns (X_train, y_train, X_test, y_test): with device=True
        torch tensors on the context's device (views of one allocation), otherwise numpy arrays.
        fe: a WaveletTransform (default (8, 512, 175, 16)); context: where the rows land (default
        the provider's first context)."""
        name, size, skip, fs = ((8, 512, 175, 16) if fe is None else
                                (fe.NAME, fe.EPOCH_SIZE, fe.SKIP_SAMPLES, fe.FEATURE_SIZE))
        n_train = ctypes.c_int64()

        def call(ctx, X, y, mem):
            args = (self._h, None if ctx is None else ctx.handle, int(seed), float(train_fraction),
                    int(name), int(size), int(skip), int(fs), _lib.ptr(X), _lib.ptr(y),
                    ctypes.byref(n_train), mem)
            if mem == _lib.MEM_DEVICE:
                ctx._call(mem, X, lib().eegfx_odp_split, *args)
            else:
                check(lib().eegfx_odp_split(*args))

        if not self._ctxs:  # planning-only: the library's refusal
            call(None, None, None, _lib.MEM_HOST)
        ctx = context if context is not None else self._ctxs[0]
        n, d = self.num_epochs(), 3 * max(int(fs), 0)
        if device:
            import torch
            buf = torch.empty(n * (d + 1), dtype=torch.float64, device=f"cuda:{ctx.device}")
            X, y = buf[:n * d].view(n, d), buf[n * d:]
            call(ctx, X, y, _lib.MEM_DEVICE)
        else:
            X, y = np.empty((n, d), dtype=np.float64), np.empty(n, dtype=np.float64)
            call(ctx, X, y, _lib.MEM_HOST)
        cut = int(n_train.value)
        return X[:cut], y[:cut], X[cut:], y[cut:]

    def splitShards(self, fe=None, seed: int = 1, train_fraction: float = 0.7
                    ) -> List[SplitShard]:
        """split() kept per shard (eegfx_odp_split_sharded): every shard's rows of the train and
        the test part stay on the shard's own context, gathered there in the order of the shuffled
        list, with their positions in it.  No feature row crosses a device boundary or reaches
        host memory.  One SplitShard per context, in shard order."""
        name, size, skip, fs = ((8, 512, 175, 16) if fe is None else
                                (fe.NAME, fe.EPOCH_SIZE, fe.SKIP_SAMPLES, fe.FEATURE_SIZE))
        k = int(lib().eegfx_odp_num_shards(self._h))
        out = (_lib.SplitShard * max(1, k))()
        check(lib().eegfx_odp_split_sharded(self._h, int(seed), float(train_fraction), int(name),
                                            int(size), int(skip), int(fs), out))
        return [SplitShard(self, out[i], 3 * int(fs), self._ctxs[i]) for i in range(k)]

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().eegfx_odp_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
