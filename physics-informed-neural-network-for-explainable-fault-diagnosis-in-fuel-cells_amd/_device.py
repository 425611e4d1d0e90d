"""What the analysis modules (risk, diagnosis, detection, comparison, anomaly, svm, embedding) share on their way to the
device: the backend="auto" rule, conversions between host arrays and device tensors, the rows of the results array read
in place (`_DevRows`, the row head of `_lib._ROWS`) with their host twin (`_host_rows`), and the launch itself (`call`).
What the supervised classifiers share on top of it (class set-up, wanted outputs, the one-vs-one base class) is _classify.py.

Importing this module needs numpy only; torch and the HIP library are loaded when a device path runs.
"""
import ctypes

import numpy as np

MAX_FEAT = 8                            # columns of a row head (csrc/pinn_rows.h: kRowsMaxD)
AUTO_DEVICE_ROWS = 50000                # backend="auto" sends a host array of at least this many rows to a present GPU


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _on_gpu(x):
    return _is_tensor(x) and x.is_cuda


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _pick_backend(backend, data, n=None, threshold=AUTO_DEVICE_ROWS):
    """The rule of backend="auto": a tensor stays where it is; a host array of `n` rows (by default its first dimension)
    goes to the device from `threshold` rows on when a GPU is present."""
    if backend not in ("auto", "device", "host"):
        raise ValueError("backend must be 'auto', 'device' or 'host'")
    if backend != "auto":
        return backend
    if _is_tensor(data):
        return "device" if data.is_cuda else "host"
    n = np.shape(data)[0] if n is None else n
    return "device" if n >= threshold and _gpu_present() else "host"


def _as_numpy(x, dtype=None):
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x) if dtype is None else np.asarray(x, dtype=dtype)


def columns_of(features, parse):
    """The column list of a monitor's `features`: a spec for `parse`, or the column numbers themselves."""
    return parse(features) if isinstance(features, str) else [int(c) for c in features]


def _host_rows(X, columns=None, row_index=None):
    a = _as_numpy(X)
    if a.ndim != 2:
        raise ValueError("X must be a 2-D array")
    if row_index is not None:
        a = a[_as_numpy(row_index, np.int64)]
    if columns is not None:
        a = a[:, list(columns)]
    return np.ascontiguousarray(a, dtype=np.float64)


def _torch_lib():
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.PinnError("the device backend of pinn_amd.risk needs a GPU (backend='host' runs on the CPU)")
    return torch, _lib, _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


_bound = None                           # (torch, _lib.check, the loaded library), bound by the first call


def call(name, *args, stream=None):
    """One call of the library's entry point `name`, on `stream` (by default torch's current one, read here): tensors go
    as their device pointers, everything else as it stands.  Raises PinnError, which names the entry point, on a failure."""
    global _bound
    if _bound is None:                  # not per call: the two imports cost as much as the rest of a launch's host side
        import torch
        from . import _lib
        _bound = (torch, _lib.check, _lib.load())
    torch, check, lib = _bound
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    check(getattr(lib, name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], stream), name)


def _dev_f64_rows(torch, data):
    """A float64 device tensor [N, ld] with unit column stride, without a copy when `data` already is one."""
    t = data if _is_tensor(data) else torch.from_numpy(np.ascontiguousarray(np.asarray(data, dtype=np.float64)))
    if t.dim() != 2:
        raise ValueError("results must be a 2-D array")
    t = t.detach().to("cuda" if not t.is_cuda else t.device, torch.float64)
    if t.shape[0] > 0 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):      # a transposed or expanded view
        t = t.contiguous()
    return t


def _dev_vec(torch, v, dtype, device):
    if v is None:
        return None
    if _is_tensor(v):
        return v.detach().to(device, dtype).reshape(-1).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1)).astype(
        np.float64 if dtype == torch.float64 else np.int64)).to(device)


class _DevRows:
    """Rows of a float64 device array read in place: column list and optional gather list."""

    def __init__(self, torch, X, columns=None, row_index=None):
        self.arr = _dev_f64_rows(torch, X)
        self.dev = self.arr.device
        cols = list(range(self.arr.shape[1])) if columns is None else [int(c) for c in columns]
        if not 1 <= len(cols) <= MAX_FEAT:
            raise ValueError("the device backend takes 1 to %d features, got %d" % (MAX_FEAT, len(cols)))
        if cols and (min(cols) < 0 or max(cols) >= self.arr.shape[1]):
            raise ValueError("X has %d columns, column %d is asked for" % (self.arr.shape[1], max(cols)))
        self.cols, self.D = cols, len(cols)
        self.c_cols = (ctypes.c_int * self.D)(*cols)
        self.ridx = _dev_vec(torch, row_index, torch.int64, self.dev)
        self.n = self.arr.shape[0] if self.ridx is None else self.ridx.numel()
        self.ld = self.arr.stride(0) if self.arr.shape[0] > 1 else max(self.arr.shape[1], 1)

    @classmethod
    def within(cls, torch, X, columns, row_index, on_excess):
        """As the constructor, but more than MAX_FEAT features are reported by the module's own `on_excess(D)`: to its
        caller a size the kernels are not built for (NotImplementedError), not a bad argument."""
        D = len(columns) if columns is not None else (int(X.shape[1]) if len(X.shape) == 2 else 1)
        if D > MAX_FEAT:
            on_excess(D)
        return cls(torch, X, columns, row_index)

    def head(self):
        return (_ptr(self.arr), self.ld, self.arr.shape[0], self.c_cols, self.D, _ptr(self.ridx), self.n)

    def packed(self, torch):
        a = self.arr if self.ridx is None else self.arr[self.ridx]
        return a[:, self.cols].contiguous()
