"""faiss-compatible surface over the MI355X flat index.

Mirrors the slice of the faiss Python API the reference uses
(faiss_store.py:29,46,64,91,106,126; rag_datastore_manager.py:138,173,186,
205,218) so a caller can switch with ``import rag_faiss_embedding_amd.faiss
as faiss``:

* ``IndexFlatL2(d)`` / ``IndexFlatIP(d)`` with ``.d``, ``.ntotal``,
  ``.metric_type``, ``.is_trained``, ``.add(x)``, ``.search(x, k) -> (D, I)``,
  ``.range_search(x, radius) -> (lims, D, I)``, ``.reset()``,
  ``.reconstruct_n(i0, n)``, ``.remove_ids(sel_or_ids) -> n_removed`` (the
  kept rows keep their order and are renumbered densely, compacted in place
  on the GPU);
* filtered search, ``index.search(x, k, params=SearchParameters(sel=...))``
  with ``IDSelectorRange``, ``IDSelectorArray``, ``IDSelectorBatch``,
  ``IDSelectorBitmap`` and ``IDSelectorNot``: only the selected ids are ranked
  (exactly: the scan itself skips the other rows);
* stable ids, ``IndexIDMap(index)`` / ``IndexIDMap2(index)`` with
  ``add_with_ids(x, ids)``, ``id_map`` and (``IndexIDMap2``)
  ``reconstruct(id)``: every row carries a caller-chosen int64 label that
  ``search`` / ``range_search`` return, selectors and ``remove_ids`` speak,
  and removals leave intact;
* stored vectors by key, on the device: ``reconstruct(key)``,
  ``reconstruct_batch(keys)``, ``search_and_reconstruct(x, k) -> (D, I, R)``
  and ``compute_distance_subset(x, labels) -> D`` (keys are the ids ``search``
  returns; one outside the index gives a NaN row / the missing slot's
  distance from device keys and raises from host keys);
* ``Kmeans(d, k, ...)`` with ``train(x)`` / ``assign(x)``, ``centroids``,
  ``obj``, ``iteration_stats`` and ``index``: k-means on the device over
  numpy rows, device tensors or a flat index's stored rows, bitwise
  reproducible;
* ``IndexScalarQuantizer(d, qtype)`` with ``QT_8bit`` / ``QT_8bit_uniform``:
  one byte per dimension, trained as min / max, searched exactly on the
  decoded rows (``train`` / ``add`` / ``search`` / ``reconstruct*`` /
  ``sa_encode`` / ``sa_decode`` / ``trained``);
* ``write_index(index, path)`` / ``read_index(path)`` on the IxF2 format
  (IxM2 for a labelled index).

Inputs may be numpy arrays (as in the reference: host fp32, results returned
as numpy) or torch tensors already resident on the GPU (fp32/bf16/fp16;
results returned as device tensors, no host round trip) -- the latter is the
device-resident hand-off from the encoder.

Errors follow faiss: a dimension mismatch raises ``AssertionError`` (the
SWIG wrapper's ``assert d == self.d``); library failures raise
``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib

METRIC_INNER_PRODUCT = _lib.METRIC_INNER_PRODUCT
METRIC_L2 = _lib.METRIC_L2

_DTYPES = {"float32": _lib.F32, "bfloat16": _lib.BF16, "float16": _lib.F16}
_DTYPE_NAMES = {v: k for k, v in _DTYPES.items()}
_UNBOUND = object()  # no stream bound yet by this Python object


def _torch():
    try:
        import torch  # noqa: F401
        return torch
    except Exception:  # pragma: no cover - torch is in the image
        return None


def _is_device_tensor(x) -> bool:
    t = _torch()
    return t is not None and isinstance(x, t.Tensor) and x.is_cuda


def _tensor_dtype(x) -> int:
    t = _torch()
    m = {t.float32: _lib.F32, t.bfloat16: _lib.BF16, t.float16: _lib.F16}
    if x.dtype not in m:
        raise TypeError(f"unsupported tensor dtype {x.dtype}")
    return m[x.dtype]


# ---------------------------------------------------------------------------
# faiss IDSelector / SearchParameters (include/fx_index.h "filtered search")
# ---------------------------------------------------------------------------
def _out_arrays(x, nq: int, k: int, D, I) -> Tuple:
    """``D`` and ``I`` of a search of the ``nq`` queries ``x``: allocated when
    None, else the caller's, checked (the C side writes nq * k elements through
    the raw pointer).  Device tensors on ``x``'s device when ``x`` is one, numpy
    arrays otherwise."""
    if _is_device_tensor(x):
        t = _torch()
        if D is None:
            D = t.empty((nq, k), dtype=t.float32, device=x.device)
        if I is None:
            I = t.empty((nq, k), dtype=t.int64, device=x.device)
        for name, a, dt in (("D", D, t.float32), ("I", I, t.int64)):
            assert _is_device_tensor(a) and a.device == x.device, f"{name} must be on {x.device}"
            assert a.dtype == dt and tuple(a.shape) == (nq, k) and a.is_contiguous(), \
                f"{name} must be a contiguous {dt} tensor of shape ({nq}, {k})"
        return D, I
    D = np.empty((nq, k), dtype=np.float32) if D is None else D
    I = np.empty((nq, k), dtype=np.int64) if I is None else I
    for name, a, dt in (("D", D, np.float32), ("I", I, np.int64)):
        assert isinstance(a, np.ndarray) and a.dtype == dt and a.shape == (nq, k) and \
            a.flags.c_contiguous and a.flags.writeable, \
            f"{name} must be a writeable C-contiguous {np.dtype(dt).name} array of shape ({nq}, {k})"
    return D, I


def _rows(self, x):
    """(pointer, dtype code, mem, n, keep-alive) of the row input ``x`` of the
    index ``self`` (whose stream is bound to match)."""
    if _is_device_tensor(x):
        assert x.dim() == 2 and x.shape[1] == self._d, "dimension mismatch"
        assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, index on cuda:{self.device}"
        x = x.contiguous()
        self._bind_stream(True)
        return ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x), _lib.MEM_DEVICE, x.shape[0], x
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 2 and x.shape[1] == self._d, "dimension mismatch"
    self._bind_stream(False)
    return x.ctypes.data_as(ctypes.c_void_p), _lib.F32, _lib.MEM_HOST, x.shape[0], x


class IDSelector:
    """A set of ids a search is restricted to.  Ids are the ids ``search``
    returns (row + the index's id offset; on a labelled index -- ``IndexIDMap``
    -- the rows' labels).  The device image a search needs
    (``FxSelector``: row mask + live tiles) is built on first use and cached
    per index for the index's current ``ntotal`` and id offset; after ``add``
    / ``reset`` / ``remove_ids`` it is rebuilt transparently."""

    _kind = -1

    def _spec(self):
        """(kind, data, n, invert): data a numpy array, a device tensor or None."""
        raise NotImplementedError

    def _handle(self, index: "_FlatIndex") -> ctypes.c_void_p:
        # id(index) -> (key, handle, library, weak reference to the index): the
        # handle goes when the index does, when it is stale, or with self
        cache = self.__dict__.setdefault("_built", {})
        key = (index.ntotal, index._id_offset, index._resets)
        hit = cache.get(id(index))
        if hit is not None and hit[0] == key:
            return hit[1]
        if hit is not None:
            del cache[id(index)]
            hit[2].fx_selector_free(hit[1])
        kind, data, n, invert = self._spec()
        h = ctypes.c_void_p()
        if _is_device_tensor(data):
            assert data.device.index == index.device, \
                f"selector data on cuda:{data.device.index}, index on cuda:{index.device}"
            ptr, mem = ctypes.c_void_p(data.data_ptr()), _lib.MEM_DEVICE
        else:
            ptr, mem = (ctypes.c_void_p(data.ctypes.data) if data is not None and data.size else None), _lib.MEM_HOST
        index._check(index._lib.fx_selector_create(index._h, kind, ptr, int(n), mem, 1 if invert else 0,
                                                   ctypes.byref(h)))
        so, iid = index._lib, id(index)

        def index_gone(_ref, cache=cache, iid=iid):
            old = cache.pop(iid, None)
            if old is not None and old[2] is not None:
                old[2].fx_selector_free(old[1])  # (valid after the index was freed)

        cache[iid] = (key, h, so, weakref.ref(index, index_gone))
        return h

    def stats(self, index: "_FlatIndex") -> dict:
        """Of this selector on ``index``: selected ``rows`` and live 128-row
        ``tiles`` (the tiles the filtered scan visits)."""
        index = _flat(index)
        index._bind_stream(_is_device_tensor(self._spec()[1]))
        r, t = ctypes.c_int64(0), ctypes.c_int64(0)
        index._check(index._lib.fx_selector_stats(self._handle(index), ctypes.byref(r), ctypes.byref(t)))
        return {"rows": r.value, "tiles": t.value}

    def __del__(self):
        try:  # (at interpreter shutdown the library or the cache may be gone already)
            built = self.__dict__.pop("_built", None) or {}
            for _, h, so, _ref in list(built.values()):
                if so is not None and h is not None and h.value:
                    so.fx_selector_free(h)
            built.clear()
        except Exception:  # noqa: BLE001
            pass


def _id_array(ids):
    if _is_device_tensor(ids):
        t = _torch()
        assert ids.dtype == t.int64, "device ids must be an int64 tensor"
        return ids.contiguous().view(-1)
    return np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)


class IDSelectorRange(IDSelector):
    """``faiss.IDSelectorRange(imin, imax)``: ids with imin <= id < imax."""

    _kind = 2

    def __init__(self, imin: int, imax: int, assume_sorted: bool = False):
        self.imin, self.imax = int(imin), int(imax)
        if self.imax < self.imin:
            raise AssertionError("IDSelectorRange: imax < imin")

    def _spec(self):
        return self._kind, np.array([self.imin, self.imax], dtype=np.int64), 2, False


class IDSelectorArray(IDSelector):
    """``faiss.IDSelectorArray(ids)``: the listed ids (duplicates and ids
    outside the index are ignored).  ``ids``: anything numpy converts to
    int64, or an int64 tensor on the index's GPU (then read stream-ordered)."""

    _kind = 1

    def __init__(self, *args):
        # faiss spells it (n, ids) in C++ and (ids) in Python
        ids = args[-1]
        self.ids = _id_array(ids)
        if len(args) == 2:
            self.ids = self.ids[:int(args[0])]

    def _spec(self):
        n = int(self.ids.numel()) if _is_device_tensor(self.ids) else int(self.ids.size)
        return self._kind, self.ids, n, False


class IDSelectorBatch(IDSelectorArray):
    """``faiss.IDSelectorBatch(ids)``: the same set as ``IDSelectorArray``
    (faiss's hash-set variant; here both build the same row mask)."""


class IDSelectorBitmap(IDSelector):
    """``faiss.IDSelectorBitmap(bitmap)`` / ``(n, bitmap)``: id i is selected
    iff ``bitmap[i >> 3] & (1 << (i & 7))``; ids past the bitmap's 8 n bits are
    not.  ``bitmap``: uint8 numpy array or uint8 tensor on the index's GPU."""

    _kind = 0

    def __init__(self, *args):
        bitmap = args[-1]
        if _is_device_tensor(bitmap):
            assert bitmap.dtype == _torch().uint8, "a device bitmap must be a uint8 tensor"
            self.bitmap = bitmap.contiguous().view(-1)
            size = int(self.bitmap.numel())
        else:
            self.bitmap = np.ascontiguousarray(np.asarray(bitmap).reshape(-1), dtype=np.uint8)
            size = int(self.bitmap.size)
        self.n = size
        if len(args) == 2:
            self.n = int(args[0])
            assert 0 <= self.n <= size, "IDSelectorBitmap: n exceeds the bitmap"

    def _spec(self):
        return self._kind, self.bitmap, self.n, False


class IDSelectorNot(IDSelector):
    """``faiss.IDSelectorNot(sel)``: the ids of the index ``sel`` does not
    select.  ``IDSelectorNot(IDSelectorNot(s))`` is ``s`` itself."""

    def __new__(cls, sel):
        if isinstance(sel, IDSelectorNot):
            return sel.sel
        return super().__new__(cls)

    def __init__(self, sel):
        if not isinstance(sel, IDSelector):
            raise TypeError("IDSelectorNot takes an IDSelector (And / Or / XOr are not supported)")
        self.sel = sel

    def _spec(self):
        kind, data, n, invert = self.sel._spec()
        return kind, data, n, not invert


class SearchParameters:
    """``faiss.SearchParameters(sel=None)``: per-search parameters; ``sel`` an
    ``IDSelector`` restricting the search, None for all rows."""

    def __init__(self, sel: Optional[IDSelector] = None):
        if sel is not None and not isinstance(sel, IDSelector):
            raise TypeError("sel must be an IDSelector")
        self.sel = sel


def _selector_of(params) -> Optional[IDSelector]:
    if params is None:
        return None
    sel = getattr(params, "sel", None)
    if sel is not None and not isinstance(sel, IDSelector):
        raise TypeError("params.sel must be an IDSelector of this module")
    return sel


class _FlatIndex:
    """Common implementation of IndexFlatL2 / IndexFlatIP."""

    _id_offset = 0
    _resets = 0  # reset() and remove_ids() calls: with ntotal and the id offset, what a built selector is a
                 # snapshot of (a removal followed by an add of as many rows restores ntotal, not the rows)

    metric_type: int = METRIC_L2
    _lib = lib  # the ctypes build this index lives in (the diagnostic build: diag.py)

    def _check(self, rc: int) -> None:
        check(rc, self._lib)

    def __init__(self, d: int, dtype: str = "float32", device: int = 0, normalize: bool = False,
                 _handle: Optional[ctypes.c_void_p] = None):
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_DTYPES)}")
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            self._check(self._lib.fx_index_create(int(d), _DTYPES[dtype], self.metric_type, int(device),
                                                  ctypes.byref(self._h)))
        self.device = int(device)
        self.storage_dtype = dtype
        self.is_trained = True
        self.verbose = False
        if normalize:
            self._check(self._lib.fx_index_set_normalize(self._h, 1))

    # -- faiss attributes ------------------------------------------------------
    @property
    def d(self) -> int:
        v = ctypes.c_int(0)
        self._check(self._lib.fx_index_dim(self._h, ctypes.byref(v)))
        return v.value

    @property
    def ntotal(self) -> int:
        v = ctypes.c_int64(0)
        self._check(self._lib.fx_index_ntotal(self._h, ctypes.byref(v)))
        return v.value

    # -- stream plumbing --------------------------------------------------------
    def _bind_stream(self, use_torch: bool) -> None:
        s = _torch().cuda.current_stream(self.device).cuda_stream if use_torch else None
        if getattr(self, "_bound", _UNBOUND) == s:  # (one C call less per search on the latency-bound path)
            return
        self._check(self._lib.fx_index_set_stream(self._h, ctypes.c_void_p(s) if s is not None else None))
        self._bound = s

    # -- add / search --------------------------------------------------------------
    def add(self, x) -> None:
        """``IndexFlat.add`` (faiss_store.py:46): append rows of ``x``."""
        if _is_device_tensor(x):
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            self._bind_stream(True)
            self._check(self._lib.fx_index_add(self._h, x.shape[0], ctypes.c_void_p(x.data_ptr()),
                                               _tensor_dtype(x), _lib.MEM_DEVICE))
            return
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
        self._bind_stream(False)
        self._check(self._lib.fx_index_add(self._h, x.shape[0], x.ctypes.data_as(ctypes.c_void_p), _lib.F32,
                                           _lib.MEM_HOST))

    def add_with_ids(self, x, ids) -> None:
        """``fx_index_add_with_ids``: append the rows of ``x``, row i labelled
        ``ids[i]`` (int64).  The thin binding ``IndexIDMap`` / ``IndexIDMap2``
        call; the first one into an empty index turns its labelled mode on."""
        dev_ids = _is_device_tensor(ids)
        ids = _id_array(ids)
        n_ids = int(ids.numel()) if dev_ids else int(ids.size)
        if dev_ids:
            assert ids.device.index == self.device, f"ids on cuda:{ids.device.index}, index on cuda:{self.device}"
            iptr, imem = ctypes.c_void_p(ids.data_ptr()), _lib.MEM_DEVICE
        else:
            iptr, imem = ctypes.c_void_p(ids.ctypes.data), _lib.MEM_HOST
        if _is_device_tensor(x):
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, index on cuda:{self.device}"
            assert n_ids == x.shape[0], f"add_with_ids: {n_ids} ids for {x.shape[0]} rows"
            x = x.contiguous()
            self._bind_stream(True)
            self._check(self._lib.fx_index_add_with_ids(self._h, x.shape[0], ctypes.c_void_p(x.data_ptr()),
                                                        _tensor_dtype(x), _lib.MEM_DEVICE, iptr, imem))
            return
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
        assert n_ids == x.shape[0], f"add_with_ids: {n_ids} ids for {x.shape[0]} rows"
        self._bind_stream(dev_ids)
        self._check(self._lib.fx_index_add_with_ids(self._h, x.shape[0], x.ctypes.data_as(ctypes.c_void_p), _lib.F32,
                                                    _lib.MEM_HOST, iptr, imem))

    @property
    def has_ids(self) -> bool:
        """True while the index is in the labelled mode (``add_with_ids``)."""
        v = ctypes.c_int(0)
        self._check(self._lib.fx_index_has_ids(self._h, ctypes.byref(v)))
        return bool(v.value)

    def get_ids(self, i0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The labels of rows ``[i0, i0 + n)`` (default: all) as numpy int64."""
        n = self.ntotal - int(i0) if n is None else int(n)
        out = np.empty(max(n, 0), dtype=np.int64)
        self._check(self._lib.fx_index_get_ids(self._h, int(i0), n, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return out

    def rows_of_ids(self, ids):
        """``fx_index_rows_of_ids``: for every label of ``ids`` the last row
        that carries it, -1 when none.  numpy in -> numpy out; an int64 tensor
        on the index's GPU in -> a device tensor out (stream-ordered)."""
        if _is_device_tensor(ids):
            t = _torch()
            ids = _id_array(ids)
            assert ids.device.index == self.device, f"ids on cuda:{ids.device.index}, index on cuda:{self.device}"
            rows = t.empty_like(ids)
            self._bind_stream(True)
            self._check(self._lib.fx_index_rows_of_ids(self._h, ctypes.c_void_p(ids.data_ptr()), int(ids.numel()),
                                                       _lib.MEM_DEVICE, ctypes.c_void_p(rows.data_ptr()),
                                                       _lib.MEM_DEVICE))
            return rows
        ids = _id_array(ids)
        rows = np.empty(ids.size, dtype=np.int64)
        self._bind_stream(False)
        self._check(self._lib.fx_index_rows_of_ids(self._h, ids.ctypes.data_as(ctypes.c_void_p), int(ids.size),
                                                   _lib.MEM_HOST, rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return rows

    def search(self, x, k: int, *, params=None, D=None, I=None) -> Tuple:
        """``IndexFlat.search`` (faiss_store.py:64): k nearest rows of every
        query row.  Returns ``(D, I)`` shaped ``(nq, k)``.  Any k, as faiss:
        k <= ``MAX_K`` runs the fused scan, larger k the exact sort path;
        slots past ntotal hold I = -1, D = +-FLT_MAX.

        ``params=SearchParameters(sel=IDSelector...)`` ranks only the selected
        ids (k <= ``MAX_K``); with fewer than k of them the remaining slots are
        missing ones.  Without a selector the call is the unfiltered one."""
        k = int(k)
        if k <= 0:
            raise AssertionError("k must be positive")
        sel = None if params is None else _selector_of(params)
        if _is_device_tensor(x):
            t = _torch()
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"queries on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            nq = x.shape[0]
            D, I = _out_arrays(x, nq, k, D, I)
            self._bind_stream(True)
            if sel is not None:
                self._check(self._lib.fx_index_search_sel(self._h, sel._handle(self), nq, ctypes.c_void_p(x.data_ptr()),
                                                          _tensor_dtype(x), _lib.MEM_DEVICE, k,
                                                          ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()),
                                                          _lib.MEM_DEVICE))
                return D, I
            self._check(self._lib.fx_index_search(self._h, nq, ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x),
                                                  _lib.MEM_DEVICE, k, ctypes.c_void_p(D.data_ptr()),
                                                  ctypes.c_void_p(I.data_ptr()), _lib.MEM_DEVICE))
            return D, I
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
        nq = x.shape[0]
        Dh, Ih = _out_arrays(x, nq, k, D, I)
        if sel is not None:
            # (a selector built from a device tensor is read on the stream that tensor was made on)
            self._bind_stream(_is_device_tensor(sel._spec()[1]))
            self._check(self._lib.fx_index_search_sel(self._h, sel._handle(self), nq, x.ctypes.data, _lib.F32,
                                                      _lib.MEM_HOST, k, Dh.ctypes.data, Ih.ctypes.data, _lib.MEM_HOST))
            return Dh, Ih
        self._bind_stream(False)
        # (raw addresses: .ctypes.data is an int, much cheaper per call than data_as)
        self._check(self._lib.fx_index_search(self._h, nq, x.ctypes.data, _lib.F32, _lib.MEM_HOST, k,
                                              Dh.ctypes.data, Ih.ctypes.data, _lib.MEM_HOST))
        return Dh, Ih

    def range_search(self, x, radius: float, *, params=None) -> Tuple:
        """``IndexFlat.range_search``: every row within ``radius`` of each
        query row -- ``D < radius`` (L2 index) or ``x.y > radius`` (IP), both
        strict, decided on the exact distance.  Returns ``(lims, D, I)``:
        query i owns ``D[lims[i]:lims[i+1]]`` / ``I[lims[i]:lims[i+1]]``,
        ordered by ascending row id.  numpy in -> numpy out (``lims`` uint64,
        as faiss); a device tensor in -> D and I device tensors and ``lims``
        an int64 tensor on the same device."""
        if _selector_of(params) is not None:
            raise NotImplementedError("range_search with an IDSelector is not supported: filtered search is "
                                      "search(x, k, params=...) only")
        radius = float(radius)
        dev_in = _is_device_tensor(x)
        if dev_in:
            t = _torch()
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"queries on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            nq, qptr, qdt, mem = x.shape[0], ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x), _lib.MEM_DEVICE
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
            nq, qptr, qdt, mem = x.shape[0], ctypes.c_void_p(x.ctypes.data), _lib.F32, _lib.MEM_HOST
        lims = np.zeros(nq + 1, dtype=np.int64)
        self._bind_stream(dev_in)
        self._check(self._lib.fx_index_range_search(self._h, nq, qptr, qdt, mem, radius,
                                                    lims.ctypes.data_as(ctypes.c_void_p)))
        total = int(lims[nq])
        if dev_in:
            D = t.empty((total,), dtype=t.float32, device=x.device)
            I = t.empty((total,), dtype=t.int64, device=x.device)
            self._check(self._lib.fx_index_range_result(self._h, ctypes.c_void_p(D.data_ptr()),
                                                        ctypes.c_void_p(I.data_ptr()), _lib.MEM_DEVICE))
            return t.from_numpy(lims).to(x.device), D, I
        D = np.empty(total, dtype=np.float32)
        I = np.empty(total, dtype=np.int64)
        self._check(self._lib.fx_index_range_result(self._h, D.ctypes.data_as(ctypes.c_void_p),
                                                    I.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return lims.astype(np.uint64), D, I

    def last_range_stats(self) -> dict:
        """Of the last ``range_search``: ``candidates`` the MFMA scan emitted
        (the exact pass kept the result's share of them) and scan ``passes``
        run (2 when the candidate buffer had to grow; 0: no scan needed)."""
        c, p = ctypes.c_int64(0), ctypes.c_int(0)
        self._check(self._lib.fx_index_last_range_stats(self._h, ctypes.byref(c), ctypes.byref(p)))
        return {"candidates": c.value, "passes": p.value}

    def last_fallbacks(self) -> int:
        """Queries of the last search whose top-k the scan's candidates could
        not certify (re-scanned with a wide candidate set)."""
        v = ctypes.c_int64(0)
        self._check(self._lib.fx_index_last_fallbacks(self._h, ctypes.byref(v)))
        return v.value

    def last_exact_fallbacks(self) -> int:
        """Of those, the queries the re-scan could not certify either,
        re-ranked by the exact fp64 scan of every row."""
        v = ctypes.c_int64(0)
        self._check(self._lib.fx_index_last_exact_fallbacks(self._h, ctypes.byref(v)))
        return v.value

    def last_scan_plan(self) -> dict:
        """The last search's scan plan: tile_rows (128 = k_scan_v4, 64 =
        k_scan_v5), query_tile (queries per workgroup), splits."""
        v = [ctypes.c_int(0) for _ in range(3)]
        self._check(self._lib.fx_index_last_scan_plan(self._h, *(ctypes.byref(x) for x in v)))
        return {"tile_rows": v[0].value, "query_tile": v[1].value, "splits": v[2].value}

    def last_dropped_candidates(self) -> int:
        """Candidate entries the last search's exact re-rank dropped for a row
        id outside [0, ntotal): 0 unless a scan list was corrupted (then the
        top-k may miss rows; treat it as an error)."""
        v = ctypes.c_int64(0)
        self._check(self._lib.fx_index_last_dropped_candidates(self._h, ctypes.byref(v)))
        return v.value

    def reset(self) -> None:
        self._check(self._lib.fx_index_reset(self._h))
        self._resets += 1

    def remove_ids(self, x) -> int:
        """``IndexFlatCodes.remove_ids``: remove the rows ``x`` selects -- an
        ``IDSelector`` of this module, or ids as ``IDSelectorBatch`` takes them
        (array-like, or an int64 tensor on the index's GPU).  The kept rows
        keep their order and are renumbered densely (row r again has id r +
        the id offset).  Returns the number of rows removed."""
        sel = x if isinstance(x, IDSelector) else IDSelectorBatch(x)
        self._bind_stream(_is_device_tensor(sel._spec()[1]))
        n = ctypes.c_int64(0)
        self._check(self._lib.fx_index_remove_ids(self._h, sel._handle(self), ctypes.byref(n)))
        if n.value:
            self._resets += 1  # every built selector, this one included, is a snapshot of the old rows
        return n.value

    def last_remove_stats(self) -> dict:
        """The plan of the last ``remove_ids`` that removed a row: ``first``
        removed row, kept rows above it moved in place (``direct_rows``) and
        through the staging buffer (``staged_rows``), ``chunks`` launched."""
        v = [ctypes.c_int64(0) for _ in range(4)]
        self._check(self._lib.fx_index_last_remove_stats(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("first", "direct_rows", "staged_rows", "chunks"), (x.value for x in v)))

    def reserve(self, n: int) -> None:
        self._check(self._lib.fx_index_reserve(self._h, int(n)))

    def reconstruct_n(self, i0: int, n: int) -> np.ndarray:
        out = np.empty((int(n), self.d), dtype=np.float32)
        self._check(self._lib.fx_index_reconstruct_n(self._h, int(i0), int(n),
                                                     out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- stored vectors by key (include/fx_index.h "stored vectors by key") --------------
    def _out_dtype(self, dtype, device_out: bool):
        """(library dtype code, numpy / torch dtype) of a read-back: fp32
        unless ``dtype="storage"`` asks for the stored bytes."""
        if dtype not in (None, "float32", "storage"):
            raise ValueError('dtype must be None, "float32" or "storage"')
        name = self.storage_dtype if dtype == "storage" else "float32"
        if device_out:
            return _DTYPES[name], getattr(_torch(), name)
        if name == "bfloat16":
            raise TypeError("numpy has no bfloat16: read bfloat16 rows back with device keys (a tensor)")
        return _DTYPES[name], np.dtype(name)

    def reconstruct_batch(self, keys, dtype=None):
        """``Index.reconstruct_batch``: the stored vectors of ``keys`` (ids as
        ``search`` returns them: row + the id offset, or labels), shape
        ``(n, d)``.  numpy (or any integer sequence) in -> numpy fp32 out, a
        key outside the index raises; an int64 tensor on the index's GPU in ->
        a device tensor out, stream-ordered, a key outside the index gives a
        NaN row.  ``dtype="storage"``: the index's storage dtype (the stored
        bytes) instead of fp32.  On a labelled index an unknown label gives a
        NaN row either way."""
        dev = _is_device_tensor(keys)
        keys = _id_array(keys)
        code, out_dt = self._out_dtype(dtype, dev)
        if dev:
            t = _torch()
            assert keys.device.index == self.device, f"keys on cuda:{keys.device.index}, index on cuda:{self.device}"
            out = t.empty((int(keys.numel()), self.d), dtype=out_dt, device=keys.device)
            self._bind_stream(True)
            self._check(self._lib.fx_index_reconstruct_batch(self._h, int(keys.numel()), ctypes.c_void_p(keys.data_ptr()),
                                                             _lib.MEM_DEVICE, ctypes.c_void_p(out.data_ptr()), code,
                                                             _lib.MEM_DEVICE))
            return out
        out = np.empty((int(keys.size), self.d), dtype=out_dt)
        self._bind_stream(False)
        self._check(self._lib.fx_index_reconstruct_batch(self._h, int(keys.size), ctypes.c_void_p(keys.ctypes.data),
                                                         _lib.MEM_HOST, ctypes.c_void_p(out.ctypes.data), code,
                                                         _lib.MEM_HOST))
        return out

    def reconstruct(self, key: int) -> np.ndarray:
        """``Index.reconstruct``: the stored vector of one id, numpy fp32."""
        return self.reconstruct_batch(np.array([int(key)], dtype=np.int64))[0]

    def search_and_reconstruct(self, x, k: int, *, params=None, dtype=None) -> Tuple:
        """``Index.search_and_reconstruct``: ``search(x, k)`` (or the filtered
        search of ``params``) and the neighbours' stored vectors: ``(D, I, R)``
        with ``R`` shaped ``(nq, k, d)``, ``R[i, j]`` the vector of the row that
        ranked j (NaN where ``I == -1``).  numpy in -> numpy out; a device
        tensor in -> device tensors out, the whole call stream-ordered.
        ``dtype="storage"``: ``R`` in the index's storage dtype."""
        k = int(k)
        if k <= 0:
            raise AssertionError("k must be positive")
        sel = None if params is None else _selector_of(params)
        dev = _is_device_tensor(x)
        code, out_dt = self._out_dtype(dtype, dev)
        if dev:
            t = _torch()
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"queries on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            nq = x.shape[0]
            D = t.empty((nq, k), dtype=t.float32, device=x.device)
            I = t.empty((nq, k), dtype=t.int64, device=x.device)
            R = t.empty((nq, k, self.d), dtype=out_dt, device=x.device)
            qptr, qdt, mem = ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x), _lib.MEM_DEVICE
            ptrs = [ctypes.c_void_p(a.data_ptr()) for a in (D, I, R)]
            self._bind_stream(True)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
            nq = x.shape[0]
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
            R = np.empty((nq, k, self.d), dtype=out_dt)
            qptr, qdt, mem = ctypes.c_void_p(x.ctypes.data), _lib.F32, _lib.MEM_HOST
            ptrs = [ctypes.c_void_p(a.ctypes.data) for a in (D, I, R)]
            # (a selector built from a device tensor is read on the stream that tensor was made on)
            self._bind_stream(sel is not None and _is_device_tensor(sel._spec()[1]))
        self._check(self._lib.fx_index_search_and_reconstruct(self._h, sel._handle(self) if sel is not None else None,
                                                              nq, qptr, qdt, mem, k, *ptrs, code, mem))
        return D, I, R

    def compute_distance_subset(self, x, labels):
        """``IndexFlat.compute_distance_subset``: ``D[i, j]`` = the exact
        distance of query row i and the stored vector of ``labels[i, j]`` (ids
        as ``search`` returns them), ``labels`` shaped ``(nq, k)``.  An id
        outside the index (-1 included) gives the missing slot's distance, so
        ``compute_distance_subset(x, I)`` reproduces the ``D`` of ``search``.
        numpy in -> numpy out; device tensors in -> a device tensor out
        (stream-ordered)."""
        dev = _is_device_tensor(x)
        if dev:
            t = _torch()
            assert x.dim() == 2 and x.shape[1] == self.d, "dimension mismatch"
            assert x.device.index == self.device, f"queries on cuda:{x.device.index}, index on cuda:{self.device}"
            assert _is_device_tensor(labels) and labels.device == x.device and labels.dtype == t.int64, \
                f"labels must be an int64 tensor on {x.device}"
            assert labels.dim() == 2 and labels.shape[0] == x.shape[0], "labels must be shaped (nq, k)"
            x, labels = x.contiguous(), labels.contiguous()
            nq, k = labels.shape
            D = t.empty((nq, k), dtype=t.float32, device=x.device)
            if nq == 0 or k == 0:
                return D
            self._bind_stream(True)
            self._check(self._lib.fx_index_compute_distance_subset(
                self._h, nq, ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x), _lib.MEM_DEVICE, k,
                ctypes.c_void_p(labels.data_ptr()), _lib.MEM_DEVICE, ctypes.c_void_p(D.data_ptr()), _lib.MEM_DEVICE))
            return D
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d, "dimension mismatch"
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        assert labels.ndim == 2 and labels.shape[0] == x.shape[0], "labels must be shaped (nq, k)"
        nq, k = labels.shape
        D = np.empty((nq, k), dtype=np.float32)
        if nq == 0 or k == 0:
            return D
        self._bind_stream(False)
        self._check(self._lib.fx_index_compute_distance_subset(
            self._h, nq, ctypes.c_void_p(x.ctypes.data), _lib.F32, _lib.MEM_HOST, k, ctypes.c_void_p(labels.ctypes.data),
            _lib.MEM_HOST, ctypes.c_void_p(D.ctypes.data), _lib.MEM_HOST))
        return D

    def set_id_offset(self, offset: int) -> None:
        self._check(self._lib.fx_index_set_id_offset(self._h, int(offset)))
        self._id_offset = int(offset)  # (built selectors are keyed on it: ids are row + offset)

    def set_option(self, name: str, value: int) -> None:
        """Per-index tuning / diagnostic option (include/fx_index.h
        ``fx_index_set_option``; defaults from the FX_* environment at creation)."""
        self._check(self._lib.fx_index_set_option(self._h, name.encode(), int(value)))

    # -- profiling (bench roofline) -------------------------------------------------
    def profile(self, enable: bool = True) -> None:
        self._check(self._lib.fx_index_profile(self._h, 1 if enable else 0))

    def profile_read(self) -> Tuple[float, float, int]:
        a, b, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._lib.fx_index_profile_read(self._h, ctypes.byref(a), ctypes.byref(b),
                                                    ctypes.byref(n)))
        return a.value, b.value, n.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.fx_index_free(h)
            self._h = ctypes.c_void_p()


class IndexFlatL2(_FlatIndex):
    """``faiss.IndexFlatL2`` (faiss_store.py:29): exact squared-L2 search."""

    metric_type = METRIC_L2


class IndexFlatIP(_FlatIndex):
    """``faiss.IndexFlatIP`` (the ``FAISS_INDEX_TYPE = "IP"`` option of
    config.py:30): exact maximum inner product search."""

    metric_type = METRIC_INNER_PRODUCT


class IndexIDMap:
    """``faiss.IndexIDMap(index)``: stable caller-chosen int64 ids over an
    ``IndexFlatL2`` / ``IndexFlatIP`` of this module, which must be empty
    ("index must be empty on input").  ``add_with_ids(x, ids)`` labels every
    row; ``search`` / ``range_search`` return the labels, selectors
    (``IDSelectorRange`` / ``Batch`` / ``Bitmap`` / ``Not``) and ``remove_ids``
    speak them, and they survive removals (the label array is compacted with
    the rows on the GPU).  Labels are any int64 -- negative, above 2^32,
    duplicated (one document id on all its chunk rows); -1 is legal but looks
    like the "missing slot" marker in results.  Results rank by (distance,
    row): ties break on insertion order, not on label.

    Unlike faiss, the labels live in the wrapped index's own C object, not in
    this wrapper: once labelled, ``self.index`` itself returns labels too (in
    faiss the inner index keeps returning row numbers)."""

    def __init__(self, index):
        if index.ntotal != 0:
            raise AssertionError("index must be empty on input")
        self.index = index

    @classmethod
    def _wrap(cls, index):
        """Around an index that is labelled already (``read_index``)."""
        self = cls.__new__(cls)
        self.index = index
        return self

    d = property(lambda self: self.index.d)
    ntotal = property(lambda self: self.index.ntotal)
    metric_type = property(lambda self: self.index.metric_type)
    is_trained = property(lambda self: self.index.is_trained)

    def add_with_ids(self, x, ids) -> None:
        """``IndexIDMap.add_with_ids``: numpy rows and ids, or device tensors
        (fp32 / bf16 / fp16 rows, int64 ids: stream-ordered)."""
        self.index.add_with_ids(x, ids)

    def add(self, x) -> None:
        raise RuntimeError("add does not make sense with IndexIDMap: use add_with_ids")

    def search(self, x, k: int, *, params=None, D=None, I=None) -> Tuple:
        """``search`` of the wrapped index; ``I`` holds labels (-1: missing)."""
        return self.index.search(x, k, params=params, D=D, I=I)

    def range_search(self, x, radius: float, *, params=None) -> Tuple:
        """``range_search`` of the wrapped index; ``I`` holds labels, ordered by
        ascending ROW within a query."""
        return self.index.range_search(x, radius, params=params)

    def search_and_reconstruct(self, x, k: int, *, params=None, dtype=None) -> Tuple:
        """``search_and_reconstruct`` of the wrapped index: ``I`` holds labels,
        ``R[i, j]`` the vector of the ROW that ranked j (labels may repeat)."""
        return self.index.search_and_reconstruct(x, k, params=params, dtype=dtype)

    def compute_distance_subset(self, x, labels):
        """``compute_distance_subset`` of the wrapped index with labels as keys
        (of a repeated label: its last row; an unknown one: the missing slot's
        distance)."""
        return self.index.compute_distance_subset(x, labels)

    def remove_ids(self, x) -> int:
        """Remove every row whose label ``x`` selects (an ``IDSelector``, or
        labels as ``IDSelectorBatch`` takes them); returns the rows removed."""
        return self.index.remove_ids(x)  # (bumps the wrapped index's _resets: built selectors are stale)

    def reset(self) -> None:
        self.index.reset()  # (... and so does this)

    @property
    def id_map(self) -> np.ndarray:
        """``IndexIDMap.id_map``: the label of every row, numpy int64 (a
        read-back from the device)."""
        if self.index.ntotal == 0:
            return np.empty(0, dtype=np.int64)
        return self.index.get_ids()


class IndexIDMap2(IndexIDMap):
    """``faiss.IndexIDMap2``: ``IndexIDMap`` plus ``reconstruct(id)`` and
    ``reconstruct_batch(ids)``."""

    def reconstruct_batch(self, labels, dtype=None):
        """The stored vectors of ``labels`` (of a repeated label: the last row
        added with it), numpy in -> numpy out, device tensor in -> device tensor
        out; an unknown label gives a NaN row (no synchronisation to find out)."""
        return self.index.reconstruct_batch(labels, dtype=dtype)

    def reconstruct(self, key: int) -> np.ndarray:
        """The stored vector of label ``key`` (of the last row added with it,
        as ``IndexIDMap2.rev_map`` keeps); an unknown label raises
        ``RuntimeError``."""
        batch = getattr(self.index, "reconstruct_batch", None)
        if batch is not None:  # one call: label -> row and the gather both on the device
            v = np.asarray(batch(np.array([int(key)], dtype=np.int64)))[0]
            if np.isnan(v).all():  # the library's answer for a label no row carries
                raise RuntimeError(f"reconstruct: key {int(key)} not found")
            return v
        # (a wrapped flat-index look-alike without the batch read-back: its row, then the row's vector)
        row = int(self.index.rows_of_ids(np.array([int(key)], dtype=np.int64))[0])
        if row < 0:
            raise RuntimeError(f"reconstruct: key {int(key)} not found")
        return self.index.reconstruct_n(row, 1)[0]


def _flat(index):
    """The flat index behind ``index`` (an ``IndexIDMap`` wraps one)."""
    return index.index if isinstance(index, IndexIDMap) else index


# ---------------------------------------------------------------------------
# faiss.Kmeans (include/fx_index.h "k-means")
# ---------------------------------------------------------------------------
KMEANS_CHUNK = 1 << 17  # rows per chunk of a k-means step (the library's default for "kmeans_chunk")


def _is_index(x) -> bool:
    return isinstance(x, (_FlatIndex, IndexIDMap))


class Kmeans:
    """``faiss.Kmeans``: Lloyd's algorithm on the GPU.  Every iteration is
    ``fx_kmeans_step`` (the centroid index's own exact k = 1 search, then the
    per-cluster fp64 sums, bitwise reproducible) and ``fx_kmeans_finish`` (the
    new centroids, faiss's empty-cluster split with a deterministic donor, the
    refill of the centroid index).

    ``train(x)`` sets ``centroids`` (numpy ``(k, d)`` fp32), ``obj`` (numpy,
    one value per iteration of the best redo), ``iteration_stats`` (a list of
    ``{"obj", "nsplit"}``), ``counts`` (numpy int64: the cluster sizes of the
    last iteration's assignment) and ``index``: an ``IndexFlatL2`` of this
    module holding the centroids (``IndexFlatIP`` when ``spherical``), stored
    in ``dtype``.

    ``x`` is a numpy array, a device tensor (fp32 / bf16 / fp16: the whole
    training is then stream-ordered, and ``obj``, ``nsplit`` and the count of
    invalid assignments are read back once, at the end), or a flat index of
    this module (``IndexFlatL2`` / ``IndexFlatIP``, or an ``IndexIDMap`` around
    one): its stored rows are the training set, gathered chunk by chunk in the
    storage dtype with ``reconstruct_batch`` on device keys, never through the
    host.  (On a labelled index the keys are the labels: of rows that share a
    label, the last one stands for all of them, as ``reconstruct`` has it.)

    Seeding follows faiss -- the training rows of a set larger than ``k *
    max_points_per_centroid`` are ``RandomState(seed).permutation(n)[:k *
    max_points_per_centroid]``, the initial centroids of redo r the first k
    rows of ``RandomState(seed + 1 + 15486557 * r).permutation(n_train)`` --
    but the generator is numpy's, not faiss's own, so a faiss run with the
    same seed starts from other rows.  The empty-cluster donor is the largest
    cluster, where faiss draws it at random.  ``kmeans_chunk`` (0: the default
    131,072) sets the rows per chunk of a step; the chunk order is part of the
    summation order."""

    def __init__(self, d: int, k: int, niter: int = 25, nredo: int = 1, verbose: bool = False,
                 spherical: bool = False, seed: int = 1234, max_points_per_centroid: int = 256,
                 min_points_per_centroid: int = 39, dtype: str = "float32", device: int = 0):
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_DTYPES)}")
        self.d, self.k = int(d), int(k)
        self.niter, self.nredo = int(niter), int(nredo)
        self.verbose, self.spherical, self.seed = bool(verbose), bool(spherical), int(seed)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.min_points_per_centroid = int(min_points_per_centroid)
        self.dtype, self.device = dtype, int(device)
        self.kmeans_chunk = 0
        self.centroids = None
        self.obj = np.empty(0, dtype=np.float64)
        self.iteration_stats = []
        self.counts = None
        self.index = None

    # -- the seeding rules (host only) --------------------------------------------
    def _subsample_rows(self, n: int) -> Optional[np.ndarray]:
        """The training rows of an n-row set: None (all of them), or the
        subsample drawn when n > k * max_points_per_centroid."""
        cap = self.k * self.max_points_per_centroid
        if n <= cap:
            return None
        return np.random.RandomState(self.seed).permutation(n)[:cap].astype(np.int64)

    def _init_rows(self, n_train: int, redo: int = 0) -> np.ndarray:
        """The training rows that are redo ``redo``'s initial centroids."""
        return np.random.RandomState(self.seed + 1 + 15486557 * redo).permutation(n_train)[:self.k].astype(np.int64)

    def _chunk(self) -> int:
        return self.kmeans_chunk if self.kmeans_chunk > 0 else KMEANS_CHUNK

    # -- the training set ---------------------------------------------------------
    def _size_of(self, x) -> int:
        if _is_index(x):
            assert x.d == self.d, "dimension mismatch"
            return x.ntotal
        assert len(x.shape) == 2 and x.shape[1] == self.d, "dimension mismatch"
        return int(x.shape[0])

    def _dev(self):
        return _torch().device("cuda", self.device)

    def _index_keys(self, x, rows: Optional[np.ndarray]):
        """Device keys of the rows of index ``x`` (all, or ``rows``)."""
        t = _torch()
        flat = _flat(x)
        n = flat.ntotal
        if flat.has_ids:
            keys = t.empty(n, dtype=t.int64, device=self._dev())
            flat._bind_stream(True)
            flat._check(flat._lib.fx_index_get_ids(flat._h, 0, n, ctypes.c_void_p(keys.data_ptr()), _lib.MEM_DEVICE))
        else:
            keys = t.arange(n, dtype=t.int64, device=self._dev()) + flat._id_offset
        return keys if rows is None else keys[t.from_numpy(rows).to(self._dev())]

    def _prepare(self, x, rows: Optional[np.ndarray]):
        """(kind, data): "host" numpy rows, "device" tensor rows, or "index"
        (flat index, device keys)."""
        t = _torch()
        if _is_index(x):
            flat = _flat(x)
            assert flat.device == self.device, f"index on cuda:{flat.device}, Kmeans on cuda:{self.device}"
            keys = self._index_keys(x, rows)
            if int(keys.numel()) <= self._chunk():  # one chunk: gathered once for all iterations
                return "device", flat.reconstruct_batch(keys, dtype="storage")
            return "index", (flat, keys)
        if _is_device_tensor(x):
            assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, Kmeans on cuda:{self.device}"
            _tensor_dtype(x)
            if rows is not None:
                x = x.index_select(0, t.from_numpy(rows).to(x.device))
            return "device", x.contiguous()
        x = np.asarray(x)
        x = np.ascontiguousarray(x, dtype=np.float16 if x.dtype == np.float16 else np.float32)
        return "host", (x if rows is None else np.ascontiguousarray(x[rows]))

    def _take(self, kind, data, rows: np.ndarray):
        """Rows ``rows`` of the prepared training set as a device tensor."""
        t = _torch()
        if kind == "index":
            flat, keys = data
            return flat.reconstruct_batch(keys[t.from_numpy(rows).to(self._dev())])
        if kind == "device":
            return data.index_select(0, t.from_numpy(rows).to(data.device))
        return t.from_numpy(np.ascontiguousarray(data[rows], dtype=np.float32)).to(self._dev())

    def _chunks(self, kind, data):
        """The prepared training set as (pointer, rows, dtype code, mem, keep-alive) pieces."""
        if kind == "host":
            code = _lib.F16 if data.dtype == np.float16 else _lib.F32
            yield ctypes.c_void_p(data.ctypes.data), data.shape[0], code, _lib.MEM_HOST, data
        elif kind == "device":
            yield ctypes.c_void_p(data.data_ptr()), data.shape[0], _tensor_dtype(data), _lib.MEM_DEVICE, data
        else:
            flat, keys = data
            step = self._chunk()
            for r0 in range(0, int(keys.numel()), step):
                xc = flat.reconstruct_batch(keys[r0:r0 + step], dtype="storage")
                yield ctypes.c_void_p(xc.data_ptr()), xc.shape[0], _tensor_dtype(xc), _lib.MEM_DEVICE, xc

    def _new_index(self):
        cls = IndexFlatIP if self.spherical else IndexFlatL2
        ix = cls(self.d, dtype=self.dtype, device=self.device)
        if self.kmeans_chunk > 0:
            ix.set_option("kmeans_chunk", self.kmeans_chunk)
        return ix

    # -- faiss surface ------------------------------------------------------------
    def train(self, x, weights=None, init_centroids=None) -> float:
        """``Kmeans.train``: returns the final objective (the sum of the squared
        distances of the last iteration's assignment; ``spherical``: of the
        inner products)."""
        if weights is not None:
            raise NotImplementedError("Kmeans.train: weights are not supported")
        n = self._size_of(x)
        if n < self.k:
            raise RuntimeError(f"Number of training points ({n}) should be at least as large as number of "
                               f"clusters ({self.k})")
        rows = self._subsample_rows(n)
        n_train = n if rows is None else int(rows.size)
        if n_train < self.k * self.min_points_per_centroid:
            import warnings
            warnings.warn(f"clustering {n_train} points to {self.k} centroids: please provide at least "
                          f"{self.k * self.min_points_per_centroid} training points", RuntimeWarning, stacklevel=2)
        if init_centroids is not None:
            init_centroids = np.array(init_centroids, dtype=np.float32, order="C")
            if init_centroids.shape != (self.k, self.d):
                raise AssertionError(f"init_centroids must have shape ({self.k}, {self.d})")
        t = _torch()
        dev = self._dev()
        kind, data = self._prepare(x, rows)
        ix = self._new_index()
        ix._bind_stream(True)
        h = ix._h
        niter, nredo = max(self.niter, 0), max(self.nredo, 1)
        sums = t.empty((self.k, self.d), dtype=t.float64, device=dev)
        counts = t.empty((nredo, self.k), dtype=t.int64, device=dev)
        obj = t.zeros((nredo, max(niter, 1)), dtype=t.float64, device=dev)
        nsplit = t.zeros((nredo, max(niter, 1)), dtype=t.int64, device=dev)
        cents = t.empty((nredo, self.k, self.d), dtype=t.float32, device=dev)
        ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
        for redo in range(nredo):
            if init_centroids is not None:
                c0 = t.from_numpy(init_centroids).to(dev)
            else:
                c0 = self._take(kind, data, self._init_rows(n_train, redo)).to(t.float32)
            if redo:
                ix.reset()
            ix.add(c0)
            cents[redo].copy_(c0)
            for it in range(niter):
                for ci, (xp, nr, code, mem, _keep) in enumerate(self._chunks(kind, data)):
                    ix._check(ix._lib.fx_kmeans_step(h, nr, xp, code, mem, None, None, ptr(sums), ptr(counts[redo]),
                                                     ptr(obj[redo, it:]), 1 if ci else 0))
                ix._check(ix._lib.fx_kmeans_finish(h, ptr(sums), ptr(counts[redo]), 1 if self.spherical else 0,
                                                   ptr(cents[redo]), ptr(nsplit[redo, it:])))
        # the one read-back: invalid assignments, objectives, repairs, centroids
        bad = ctypes.c_int64(0)
        ix._check(ix._lib.fx_kmeans_status(h, ctypes.byref(bad)))
        obj_h, nsplit_h = obj.cpu().numpy()[:, :niter], nsplit.cpu().numpy()[:, :niter]
        best = 0
        if niter > 0 and nredo > 1:
            final = obj_h[:, -1]
            best = int(np.argmax(final) if self.spherical else np.argmin(final))
            if best != nredo - 1:
                ix.reset()
                ix.add(cents[best])
        self.index = ix
        self.centroids = cents[best].cpu().numpy()
        self.counts = counts[best].cpu().numpy() if niter > 0 else None
        self.obj = obj_h[best].copy()
        self.iteration_stats = [{"obj": float(o), "nsplit": int(s)} for o, s in zip(obj_h[best], nsplit_h[best])]
        if self.verbose:
            for i, st in enumerate(self.iteration_stats):
                print(f"  Iteration {i} objective={st['obj']:g} nsplit={st['nsplit']}")
        return float(self.obj[-1]) if niter > 0 else 0.0

    def assign(self, x) -> Tuple:
        """``Kmeans.assign``: ``(D, I)``, two 1-D arrays: the distance to and
        the number of the nearest centroid of every row (numpy in -> numpy
        out, a device tensor in -> device tensors out, an index in -> numpy,
        in row order)."""
        assert self.index is not None, "should train before assigning"
        if not _is_index(x):
            D, I = self.index.search(x, 1)
            return D.reshape(-1), I.reshape(-1)
        t = _torch()
        flat, keys = _flat(x), self._index_keys(x, None)
        n = int(keys.numel())
        D = t.empty((n, 1), dtype=t.float32, device=keys.device)
        I = t.empty((n, 1), dtype=t.int64, device=keys.device)
        step = self._chunk()
        for r0 in range(0, n, step):
            xc = flat.reconstruct_batch(keys[r0:r0 + step], dtype="storage")
            self.index.search(xc, 1, D=D[r0:r0 + step], I=I[r0:r0 + step])
        return D.reshape(-1).cpu().numpy(), I.reshape(-1).cpu().numpy()


# ---------------------------------------------------------------------------
# faiss.IndexIVFFlat (include/fx_index.h "inverted file")
# ---------------------------------------------------------------------------
class SearchParametersIVF(SearchParameters):
    """``faiss.SearchParametersIVF(nprobe=1)``: per-search parameters of an
    ``IndexIVFFlat``.  A selector (``sel``) is accepted here as in faiss but
    the IVF search does not take one (``NotImplementedError``)."""

    def __init__(self, sel: Optional[IDSelector] = None, nprobe: int = 1):
        super().__init__(sel)
        self.nprobe = int(nprobe)


class IndexIVFFlat:
    """``faiss.IndexIVFFlat(quantizer, d, nlist, metric)``: rows live in
    ``nlist`` inverted lists, row i in list ``quantizer.search(x_i, 1)``; a
    search ranks only the rows of the ``nprobe`` lists ``quantizer.search(q,
    nprobe)`` names.  Within those lists the result is exact as the flat
    index's is (ids bit-exact, distances the fp64 sum rounded once), ranked by
    (distance, list number, insertion order within the list); with ``nprobe =
    nlist`` it reproduces the flat index.

    ``quantizer`` is an unlabelled ``IndexFlatL2`` / ``IndexFlatIP`` of this
    module on the same device; this object keeps it alive.  ``is_trained`` is
    True as soon as ``quantizer.ntotal == nlist``, so centroids saved with
    ``write_index(quantizer)`` and read back make a trained index.

    ``train(x)`` on an untrained index runs this module's ``Kmeans(d, nlist,
    niter, seed, max_points_per_centroid=256)`` -- L2 Lloyd iterations, which
    is what faiss does for the level-1 quantizer as remembered; it is not
    checked against a faiss build -- and adds the centroids to the quantizer.

    Not offered: ``write_index`` / ``read_index`` of the IVF index itself
    (persist the quantizer and re-add), ``remove_ids``, ``range_search``,
    selectors, ``reconstruct*``, ``search_preassigned``."""

    def __init__(self, quantizer, d: int, nlist: int, metric: int = METRIC_L2, dtype: str = "float32",
                 device: int = 0, niter: int = 10, seed: int = 1234):
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_DTYPES)}")
        assert isinstance(quantizer, _FlatIndex), "quantizer must be an IndexFlatL2 / IndexFlatIP of this module"
        assert quantizer.d == int(d), f"quantizer has d = {quantizer.d}, the index d = {int(d)}"
        assert quantizer.device == int(device), f"quantizer on cuda:{quantizer.device}, index on cuda:{int(device)}"
        assert metric in (METRIC_L2, METRIC_INNER_PRODUCT), "metric must be METRIC_L2 or METRIC_INNER_PRODUCT"
        self.quantizer = quantizer
        self._lib = quantizer._lib
        self._d, self.nlist, self.metric_type = int(d), int(nlist), int(metric)
        self.storage_dtype, self.device = dtype, int(device)
        self.nprobe = 1
        self.niter, self.seed = int(niter), int(seed)
        self.verbose = False
        self._mode = None  # "seq" (add) or "ids" (add_with_ids) while the index holds rows
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(quantizer._h, self._d, self.nlist, _DTYPES[dtype], self.metric_type,
                                       ctypes.byref(self._h)))

    _PFX = "fx_ivf_"  # the C entry points of this class (IndexIVFScalarQuantizer: its own set)

    def _fn(self, name: str):
        return getattr(self._lib, self._PFX + name)

    def _check(self, rc: int) -> None:
        check(rc, self._lib)

    @property
    def d(self) -> int:
        return self._d

    @property
    def ntotal(self) -> int:
        v = ctypes.c_int64(0)
        self._check(self._fn("ntotal")(self._h, ctypes.byref(v)))
        return v.value

    @property
    def is_trained(self) -> bool:
        return self.quantizer.ntotal == self.nlist

    def _bind_stream(self, use_torch: bool) -> None:
        s = _torch().cuda.current_stream(self.device).cuda_stream if use_torch else None
        if getattr(self, "_bound", _UNBOUND) == s:
            return
        self._check(self._fn("set_stream")(self._h, ctypes.c_void_p(s) if s is not None else None))
        self._bound = s

    def train(self, x) -> None:
        """Train the coarse quantizer (a no-op on a trained index, as faiss)."""
        if self.is_trained:
            return
        assert self.quantizer.ntotal == 0, "the quantizer holds rows but not nlist of them"
        km = Kmeans(self._d, self.nlist, niter=self.niter, seed=self.seed, max_points_per_centroid=256,
                    dtype=self.quantizer.storage_dtype, device=self.device)
        km.train(x)
        self.quantizer.add(km.centroids)

    def _add(self, x, ids) -> None:
        assert self.is_trained, "the index is not trained"
        mode = "seq" if ids is None else "ids"
        if self.ntotal > 0 and self._mode is not None and mode != self._mode:
            raise AssertionError("add does not make sense on an index with labels: use add_with_ids" if mode == "seq"
                                 else "add_with_ids not implemented for an index that holds rows without labels")
        iptr, imem, dev_ids, n_ids = None, _lib.MEM_HOST, False, None
        if ids is not None:
            dev_ids = _is_device_tensor(ids)
            ids = _id_array(ids)
            n_ids = int(ids.numel()) if dev_ids else int(ids.size)
            if dev_ids:
                assert ids.device.index == self.device, f"ids on cuda:{ids.device.index}, index on cuda:{self.device}"
                iptr, imem = ctypes.c_void_p(ids.data_ptr()), _lib.MEM_DEVICE
            else:
                iptr = ctypes.c_void_p(ids.ctypes.data)
        if _is_device_tensor(x):
            assert x.dim() == 2 and x.shape[1] == self._d, "dimension mismatch"
            assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            xptr, code, mem, n = ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x), _lib.MEM_DEVICE, x.shape[0]
            self._bind_stream(True)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 2 and x.shape[1] == self._d, "dimension mismatch"
            xptr, code, mem, n = x.ctypes.data_as(ctypes.c_void_p), _lib.F32, _lib.MEM_HOST, x.shape[0]
            self._bind_stream(dev_ids)
        assert n_ids is None or n_ids == n, f"add_with_ids: {n_ids} ids for {n} rows"
        self._check(self._fn("add")(self._h, n, xptr, code, mem, iptr, imem))
        if n > 0:
            self._mode = mode

    def add(self, x) -> None:
        """Append the rows of ``x`` with ids ``ntotal .. ntotal + n - 1``."""
        self._add(x, None)

    def add_with_ids(self, x, ids) -> None:
        """Append the rows of ``x``, row i with id ``ids[i]`` (any int64)."""
        self._add(x, ids)

    def add_from_index(self, index) -> None:
        """Append the stored rows of an unlabelled flat index of this module
        with ids equal to their row numbers there (``add_with_ids``), gathered
        chunk by chunk in the storage dtype on the device, never through the
        host."""
        t = _torch()
        flat = _flat(index)
        assert not flat.has_ids and flat.device == self.device and flat.d == self._d
        n = flat.ntotal
        for r0 in range(0, n, KMEANS_CHUNK):
            keys = t.arange(r0, min(n, r0 + KMEANS_CHUNK), dtype=t.int64, device=t.device("cuda", self.device))
            self.add_with_ids(flat.reconstruct_batch(keys + flat._id_offset, dtype="storage"), keys)

    def _nprobe_of(self, params) -> int:
        nprobe = self.nprobe
        if params is not None:
            if _selector_of(params) is not None:
                raise NotImplementedError(f"{type(self).__name__}.search takes no selector")
            nprobe = getattr(params, "nprobe", nprobe)
        nprobe = int(nprobe)
        if nprobe < 1:
            raise AssertionError("nprobe must be positive")
        return min(nprobe, self.nlist)

    def search(self, x, k: int, *, params=None, D=None, I=None) -> Tuple:
        """The k best rows of every query among its ``nprobe`` probed lists
        (``self.nprobe``, or ``params=SearchParametersIVF(nprobe=...)``; at most
        ``nlist``).  numpy in -> numpy out (blocks); device tensors in -> device
        tensors out, stream-ordered (the first search after an add may
        synchronise once for the regroup).  ``k > MAX_K``: NotImplementedError.

        ``k <= 32`` takes the fused path (MFMA list scan + exact refine), larger
        k the exact list scan.  Limitation: the refine certifies a query from
        the room between its k-th and its 32nd candidate, so as k nears 32 more
        queries fall to the exact list scan (at k = 32 every query whose probed
        lists hold 32 rows or more): correct, but much slower than small k
        (``last_fallbacks()`` counts them)."""
        k = int(k)
        if k <= 0:
            raise AssertionError("k must be positive")
        nprobe = self._nprobe_of(params)
        assert self.is_trained, "the index is not trained"
        if k > _lib.MAX_K:
            raise NotImplementedError(f"{type(self).__name__}.search: k = {k} above MAX_K = {_lib.MAX_K}")
        if _is_device_tensor(x):
            t = _torch()
            assert x.dim() == 2 and x.shape[1] == self._d, "dimension mismatch"
            assert x.device.index == self.device, f"queries on cuda:{x.device.index}, index on cuda:{self.device}"
            x = x.contiguous()
            nq = x.shape[0]
            D, I = _out_arrays(x, nq, k, D, I)
            self._bind_stream(True)
            self._check(self._fn("search")(self._h, nq, ctypes.c_void_p(x.data_ptr()), _tensor_dtype(x),
                                           _lib.MEM_DEVICE, k, nprobe, ctypes.c_void_p(D.data_ptr()),
                                           ctypes.c_void_p(I.data_ptr()), _lib.MEM_DEVICE))
            return D, I
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self._d, "dimension mismatch"
        nq = x.shape[0]
        Dh, Ih = _out_arrays(x, nq, k, D, I)
        self._bind_stream(False)
        self._check(self._fn("search")(self._h, nq, x.ctypes.data, _lib.F32, _lib.MEM_HOST, k, nprobe,
                                       Dh.ctypes.data, Ih.ctypes.data, _lib.MEM_HOST))
        return Dh, Ih

    def reset(self) -> None:
        """Empties the lists; the quantizer (the training) stays, as in faiss."""
        self._check(self._fn("reset")(self._h))
        self._mode = None

    def list_sizes(self) -> np.ndarray:
        out = np.zeros(self.nlist, dtype=np.int64)
        self._check(self._fn("list_sizes")(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def get_list_ids(self, l: int) -> np.ndarray:
        """The ids of list ``l`` in insertion order (numpy int64)."""
        n = ctypes.c_int64(0)
        self._check(self._fn("list_ids")(self._h, int(l), None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._check(self._fn("list_ids")(self._h, int(l), out.ctypes.data_as(ctypes.c_void_p), n.value,
                                             ctypes.byref(n)))
        return out

    def _counts(self):
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._fn("last_counts")(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def last_fallbacks(self) -> int:
        return self._counts()[0]

    def last_exact_fallbacks(self) -> int:
        return self._counts()[1]

    def last_dropped_candidates(self) -> int:
        return self._counts()[2]

    def profile(self, enable: bool = True) -> None:
        """Record HIP events around the parts of every search pass."""
        self._check(self._fn("profile")(self._h, 1 if enable else 0))

    def profile_read(self) -> dict:
        """Milliseconds since the last read (waits for the stream): ``coarse``,
        ``pairs`` (+ query preparation), ``scan`` (the list scan), ``refine``
        (+ exact fallback), and the ``passes`` they cover."""
        ms = [ctypes.c_double(0) for _ in range(4)]
        n = ctypes.c_int64(0)
        self._check(self._fn("profile_read")(self._h, *(ctypes.byref(m) for m in ms), ctypes.byref(n)))
        return {"coarse": ms[0].value, "pairs": ms[1].value, "scan": ms[2].value, "refine": ms[3].value,
                "passes": n.value}

    def last_ivf_plan(self) -> dict:
        """The planner's outputs for the last search: ``path`` ("fused" /
        "exact"), ``chunks`` per list, ``slots`` per query, ``q_batch``,
        ``grid`` (the list scan's launch bound)."""
        p, c, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        qb, g = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._fn("last_plan")(self._h, ctypes.byref(p), ctypes.byref(c), ctypes.byref(s),
                                          ctypes.byref(qb), ctypes.byref(g)))
        return {"path": "exact" if p.value else "fused", "chunks": c.value, "slots": s.value, "q_batch": qb.value,
                "grid": g.value}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._fn("free")(h)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass
            self._h = None


# ---------------------------------------------------------------------------
# faiss.IndexScalarQuantizer (include/fx_index.h "scalar quantizer")
# ---------------------------------------------------------------------------
class ScalarQuantizer:
    """faiss's ``ScalarQuantizer.QT_*`` numbers."""

    QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16 = 0, 1, 2, 3, 4
    QT_8bit_direct, QT_6bit, QT_bf16, QT_8bit_direct_signed = 5, 6, 7, 8


_QT_NAMES = {v: k for k, v in vars(ScalarQuantizer).items() if k.startswith("QT_")}


class _CodeIndex:
    """What ``IndexScalarQuantizer`` and ``IndexPQ`` share: a flat index of
    8-bit codes behind the C entry points ``_PFX + name``, searched as its
    decoded rows.  A subclass sets ``_PFX``, ``_CODE_DIM`` (the code width's
    name in messages) and ``code_size``, names ``_last_plan`` as faiss-side
    users know it, creates the handle and trains."""

    _lib = lib
    _PFX = _CODE_DIM = None

    def _fn(self, name: str):
        return getattr(self._lib, self._PFX + name)

    def _check(self, rc: int) -> None:
        check(rc, self._lib)

    @property
    def d(self) -> int:
        return self._d

    @property
    def ntotal(self) -> int:
        v = ctypes.c_int64(0)
        self._check(self._fn("ntotal")(self._h, ctypes.byref(v)))
        return v.value

    @property
    def is_trained(self) -> bool:
        v = ctypes.c_int(0)
        self._check(self._fn("is_trained")(self._h, ctypes.byref(v)))
        return bool(v.value)

    def _bind_stream(self, use_torch: bool) -> None:
        s = _torch().cuda.current_stream(self.device).cuda_stream if use_torch else None
        if getattr(self, "_bound", _UNBOUND) == s:
            return
        self._check(self._fn("set_stream")(self._h, ctypes.c_void_p(s) if s is not None else None))
        self._bound = s

    _rows = _rows

    def _chunks_of(self, index):
        """The stored rows of an unlabelled flat index of this module, chunk by
        chunk as device tensors in its storage dtype (never through the host)."""
        t = _torch()
        flat = _flat(index)
        assert not flat.has_ids and flat.device == self.device and flat.d == self._d
        n = flat.ntotal
        for r0 in range(0, n, KMEANS_CHUNK):
            keys = t.arange(r0, min(n, r0 + KMEANS_CHUNK), dtype=t.int64, device=t.device("cuda", self.device))
            yield flat.reconstruct_batch(keys + flat._id_offset, dtype="storage")

    def add(self, x) -> None:
        """Encode and append the rows of ``x`` with ids ``ntotal .. ntotal + n - 1``."""
        assert self.is_trained, "the index is not trained"
        ptr, code, mem, n, _keep = self._rows(x)
        self._check(self._fn("add")(self._h, n, ptr, code, mem))

    def add_from_index(self, index) -> None:
        """Encode and append the stored rows of an unlabelled flat index of this
        module in their order, gathered chunk by chunk on the device."""
        for rows in self._chunks_of(index):
            self.add(rows)

    def search(self, x, k: int, *, params=None, D=None, I=None) -> Tuple:
        """The k nearest decoded rows of every query.  numpy in -> numpy out
        (blocks); device tensors in -> device tensors out, stream-ordered.
        ``k <= 32`` takes the fused path (``IndexScalarQuantizer``: the int8
        MFMA scan; ``IndexPQ``, with ``dsub % 8 == 0``: the gather scan on the
        bf16 MFMA; then the exact refine), anything else the exact scan
        (correct, one fp64 pass over every row); ``k > MAX_K``:
        NotImplementedError."""
        k = int(k)
        if k <= 0:
            raise AssertionError("k must be positive")
        name = type(self).__name__
        if params is not None and _selector_of(params) is not None:
            raise NotImplementedError(f"{name}.search takes no selector")
        assert self.is_trained, "the index is not trained"
        if k > _lib.MAX_K:
            raise NotImplementedError(f"{name}.search: k = {k} above MAX_K = {_lib.MAX_K}")
        ptr, code, mem, nq, _keep = self._rows(x)
        D, I = _out_arrays(x, nq, k, D, I)
        if mem == _lib.MEM_DEVICE:
            self._check(self._fn("search")(self._h, nq, ptr, code, mem, k, ctypes.c_void_p(D.data_ptr()),
                                           ctypes.c_void_p(I.data_ptr()), mem))
        else:
            self._check(self._fn("search")(self._h, nq, ptr, code, mem, k, D.ctypes.data, I.ctypes.data, mem))
        return D, I

    def reconstruct_n(self, i0: int = 0, n: int = -1) -> np.ndarray:
        """The decoded rows ``[i0, i0 + n)`` as numpy fp32 (n = -1: to the end)."""
        i0 = int(i0)
        n = self.ntotal - i0 if int(n) < 0 else int(n)
        out = np.empty((n, self._d), dtype=np.float32)
        self._bind_stream(False)
        self._check(self._fn("reconstruct_n")(self._h, i0, n, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return out

    def reconstruct_batch(self, keys):
        """The decoded rows of ``keys``: numpy in -> numpy fp32 out (a key
        outside the index raises); an int64 device tensor in -> a device tensor
        out, stream-ordered (a key outside the index gives a NaN row)."""
        if _is_device_tensor(keys):
            t = _torch()
            keys = keys.to(t.int64).contiguous().reshape(-1)
            out = t.empty((int(keys.numel()), self._d), dtype=t.float32, device=keys.device)
            self._bind_stream(True)
            self._check(self._fn("reconstruct_batch")(self._h, int(keys.numel()), ctypes.c_void_p(keys.data_ptr()),
                                                      _lib.MEM_DEVICE, ctypes.c_void_p(out.data_ptr()), _lib.MEM_DEVICE))
            return out
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        n = self.ntotal
        if keys.size and (keys.min() < 0 or keys.max() >= n):
            raise RuntimeError(f"reconstruct_batch: a key outside [0, {n})")
        out = np.empty((int(keys.size), self._d), dtype=np.float32)
        self._bind_stream(False)
        self._check(self._fn("reconstruct_batch")(self._h, int(keys.size), ctypes.c_void_p(keys.ctypes.data),
                                                  _lib.MEM_HOST, ctypes.c_void_p(out.ctypes.data), _lib.MEM_HOST))
        return out

    def reconstruct(self, key: int) -> np.ndarray:
        return self.reconstruct_batch(np.array([int(key)], dtype=np.int64))[0]

    def sa_encode(self, x):
        """Rows -> faiss's codes ``(n, code_size)`` uint8 (a scalar quantizer's
        are unsigned; numpy in -> numpy out; a device tensor in -> a device
        tensor out)."""
        ptr, code, mem, n, _keep = self._rows(x)
        if mem == _lib.MEM_DEVICE:
            t = _torch()
            out = t.empty((n, self.code_size), dtype=t.uint8, device=_keep.device)
            self._check(self._fn("encode")(self._h, n, ptr, code, ctypes.c_void_p(out.data_ptr()), mem))
            return out
        out = np.empty((n, self.code_size), dtype=np.uint8)
        self._check(self._fn("encode")(self._h, n, ptr, code, ctypes.c_void_p(out.ctypes.data), mem))
        return out

    def sa_decode(self, codes):
        """faiss's codes ``(n, code_size)`` uint8 -> fp32 rows."""
        cs, what = self.code_size, f"codes must be (n, {self._CODE_DIM}) uint8"
        if _is_device_tensor(codes):
            t = _torch()
            assert codes.dtype == t.uint8 and codes.dim() == 2 and codes.shape[1] == cs, what
            codes = codes.contiguous()
            out = t.empty((codes.shape[0], self._d), dtype=t.float32, device=codes.device)
            self._bind_stream(True)
            self._check(self._fn("decode")(self._h, codes.shape[0], ctypes.c_void_p(codes.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), _lib.MEM_DEVICE))
            return out
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == cs, what
        out = np.empty((codes.shape[0], self._d), dtype=np.float32)
        self._bind_stream(False)
        self._check(self._fn("decode")(self._h, codes.shape[0], ctypes.c_void_p(codes.ctypes.data),
                                       ctypes.c_void_p(out.ctypes.data), _lib.MEM_HOST))
        return out

    def reset(self) -> None:
        """Empties the index; the training stays, as in faiss."""
        self._check(self._fn("reset")(self._h))

    def _counts(self):
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._fn("last_counts")(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def last_fallbacks(self) -> int:
        return self._counts()[0]

    def last_exact_fallbacks(self) -> int:
        return self._counts()[1]

    def last_dropped_candidates(self) -> int:
        return self._counts()[2]

    def _last_plan(self) -> dict:
        """The planner's outputs for the last search: ``path`` ("fused" /
        "exact"), ``qtiles`` per pass, corpus ``splits`` per query tile,
        ``xsplits`` of the exact scan, ``q_batch``, ``grid``."""
        p, t_, s, x = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        qb, g = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._fn("last_plan")(self._h, ctypes.byref(p), ctypes.byref(t_), ctypes.byref(s),
                                          ctypes.byref(x), ctypes.byref(qb), ctypes.byref(g)))
        return {"path": "exact" if p.value else "fused", "qtiles": t_.value, "splits": s.value, "xsplits": x.value,
                "q_batch": qb.value, "grid": g.value}

    def profile(self, enable: bool = True) -> None:
        """Record HIP events around the parts of every search pass."""
        self._check(self._fn("profile")(self._h, 1 if enable else 0))

    def profile_read(self) -> dict:
        """Milliseconds since the last read (waits for the stream): ``prep``,
        ``scan``, ``refine`` (+ exact fallback), and the ``passes`` they cover."""
        ms = [ctypes.c_double(0) for _ in range(3)]
        n = ctypes.c_int64(0)
        self._check(self._fn("profile_read")(self._h, *(ctypes.byref(m) for m in ms), ctypes.byref(n)))
        return {"prep": ms[0].value, "scan": ms[1].value, "refine": ms[2].value, "passes": n.value}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._fn("free")(h)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass
            self._h = None


class IndexScalarQuantizer(_CodeIndex):
    """``faiss.IndexScalarQuantizer(d, qtype, metric)`` with 8-bit codes: one
    byte per dimension after a per-dimension (``QT_8bit``) or global
    (``QT_8bit_uniform``) affine quantisation trained as min / max.  A search
    ranks the DECODED vectors (``reconstruct``) exactly as the flat index
    ranks its rows: ids bit-exact, distances the fp64 sum rounded once, ties
    to the smaller row; ids are row numbers in insertion order.  The
    definition restates faiss's from memory and is not checked against a
    faiss build.

    Not offered: the other qtypes (``NotImplementedError``), selectors,
    ``remove_ids``, ``range_search``, ``IndexIDMap`` over it, ``write_index``
    / ``read_index``."""

    _PFX, _CODE_DIM = "fx_sq_", "d"

    def __init__(self, d: int, qtype: int = ScalarQuantizer.QT_8bit, metric: int = METRIC_L2, device: int = 0):
        qtype = int(qtype)
        if qtype not in (ScalarQuantizer.QT_8bit, ScalarQuantizer.QT_8bit_uniform):
            name = _QT_NAMES.get(qtype, f"qtype {qtype}")
            hint = ""
            if qtype in (ScalarQuantizer.QT_fp16, ScalarQuantizer.QT_bf16):
                hint = (": use the flat index with dtype=\"float16\"" if qtype == ScalarQuantizer.QT_fp16
                        else ": use the flat index with dtype=\"bfloat16\"")
            raise NotImplementedError(f"IndexScalarQuantizer: {name} is not offered (QT_8bit, QT_8bit_uniform){hint}")
        assert metric in (METRIC_L2, METRIC_INNER_PRODUCT), "metric must be METRIC_L2 or METRIC_INNER_PRODUCT"
        self._d, self.qtype, self.metric_type, self.device = int(d), qtype, int(metric), int(device)
        self._lib = self._lib  # the build this handle belongs to, for its whole life
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(self._d, qtype, self.metric_type, self.device, ctypes.byref(self._h)))

    @property
    def code_size(self) -> int:
        return self._d

    def train(self, x) -> None:
        """Per-dimension (``QT_8bit_uniform``: global) min and max of ``x``:
        numpy rows, a device tensor, or a flat index of this module (its
        stored rows, gathered on the device chunk by chunk).  Non-finite
        values fail the training."""
        assert self.ntotal == 0, "train on an index that holds rows: reset() it first"
        if _is_index(x):
            for rows in self._chunks_of(x):
                ptr, code, mem, n, _keep = self._rows(rows)
                self._check(self._fn("train")(self._h, n, ptr, code, mem, 1))
            self._check(self._fn("train")(self._h, 0, None, _lib.F32, _lib.MEM_DEVICE, 0))
            return
        ptr, code, mem, n, _keep = self._rows(x)
        self._check(self._fn("train")(self._h, n, ptr, code, mem, 0))

    @property
    def trained(self) -> np.ndarray:
        """faiss's ``sq.trained``: ``[vmin[d] | vdiff[d]]`` fp32 (``QT_8bit_uniform``:
        ``[vmin, vdiff]``)."""
        out = np.empty(2 * self._d, dtype=np.float32)
        self._check(self._fn("get_trained")(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        if self.qtype == ScalarQuantizer.QT_8bit_uniform:
            return np.array([out[0], out[self._d]], dtype=np.float32)
        return out

    def set_trained(self, arr) -> None:
        """Install a training kept with numpy (the array ``trained`` returned)."""
        assert self.ntotal == 0, "set_trained on an index that holds rows: reset() it first"
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        if self.qtype == ScalarQuantizer.QT_8bit_uniform and a.size == 2:
            a = np.concatenate([np.full(self._d, a[0], np.float32), np.full(self._d, a[1], np.float32)])
        assert a.size == 2 * self._d, f"trained must hold {2 * self._d} floats"
        self._check(self._fn("set_trained")(self._h, a.ctypes.data_as(ctypes.c_void_p)))

    last_sq_plan = _CodeIndex._last_plan


# ---------------------------------------------------------------------------
# faiss.IndexPQ (include/fx_index.h "product quantizer")
# ---------------------------------------------------------------------------
class ProductQuantizer:
    """faiss's ``index.pq``: the shape of the quantizer (``M`` sub-quantizers of
    ``dsub`` dimensions, ``ksub`` = 256 centroids each, ``code_size`` = M bytes)
    and its ``centroids``, faiss's flat ``M * ksub * dsub`` fp32 array (get and
    set; setting them installs the training).  ``niter`` and ``seed`` are the
    k-means parameters ``IndexPQ.train`` uses."""

    def __init__(self, index, d: int, M: int, nbits: int, niter: int, seed: int):
        self._index = index
        self.d, self.M, self.nbits = int(d), int(M), int(nbits)
        self.dsub, self.ksub = self.d // self.M, 1 << self.nbits
        self.code_size = self.M
        self.niter, self.seed = int(niter), int(seed)

    @property
    def centroids(self) -> np.ndarray:
        ix = self._index
        out = np.empty(self.M * self.ksub * self.dsub, dtype=np.float32)
        ix._check(ix._fn("get_centroids")(ix._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    @centroids.setter
    def centroids(self, arr) -> None:
        ix = self._index
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        assert a.size == self.M * self.ksub * self.dsub, f"centroids must hold {self.M * self.ksub * self.dsub} floats"
        assert ix.ntotal == 0, "centroids set on an index that holds rows: reset() it first"
        ix._check(ix._fn("set_centroids")(ix._h, a.ctypes.data_as(ctypes.c_void_p)))


class IndexPQ(_CodeIndex):
    """``faiss.IndexPQ(d, M, nbits, metric)`` with 8-bit codes: M bytes per row,
    byte m naming one of the 256 centroids of sub-quantizer m; a row decodes to
    the concatenation of its centroids (``reconstruct``, bitwise).  A search
    ranks the DECODED vectors exactly as the flat index ranks its rows: ids
    bit-exact, distances the fp64 sum rounded once, ties (rows with equal
    codes) to the smaller row; ids are row numbers in insertion order.  The
    definition restates faiss's from memory and is not checked against a faiss
    build.

    Not offered: ``nbits != 8`` (``NotImplementedError``), selectors,
    ``remove_ids``, ``range_search``, ``IndexIDMap`` over it, ``write_index`` /
    ``read_index``."""

    _PFX, _CODE_DIM = "fx_pq_", "M"

    def __init__(self, d: int, M: int, nbits: int = 8, metric: int = METRIC_L2, device: int = 0, niter: int = 25,
                 seed: int = 1234):
        d, M, nbits = int(d), int(M), int(nbits)
        if nbits != 8:
            raise NotImplementedError(f"IndexPQ: nbits = {nbits} is not offered (8)")
        if d <= 0 or M <= 0 or d % M != 0:
            raise ValueError(f"IndexPQ: d = {d} is not a multiple of M = {M}")
        assert metric in (METRIC_L2, METRIC_INNER_PRODUCT), "metric must be METRIC_L2 or METRIC_INNER_PRODUCT"
        self._d, self.metric_type, self.device = d, int(metric), int(device)
        self.pq = ProductQuantizer(self, d, M, nbits, niter, seed)
        self._lib = self._lib  # the build this handle belongs to, for its whole life
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(d, M, nbits, self.metric_type, self.device, ctypes.byref(self._h)))

    @property
    def code_size(self) -> int:
        return self.pq.M

    def train(self, x) -> None:
        """``Kmeans(dsub, 256, niter=pq.niter, seed=pq.seed)`` on the contiguous
        slice ``x[:, m * dsub:(m + 1) * dsub]`` of every sub-quantizer m, the
        centroids then installed as ``pq.centroids``.  ``x``: numpy rows, a
        device tensor, or a flat index of this module (its stored rows,
        gathered on the device chunk by chunk).  Fewer than 256 rows is an
        error."""
        assert self.ntotal == 0, "train on an index that holds rows: reset() it first"
        pq = self.pq
        if _is_index(x):
            t = _torch()
            chunks = list(self._chunks_of(x))
            n = sum(int(c.shape[0]) for c in chunks)

            def piece(m):
                return t.cat([c[:, m * pq.dsub:(m + 1) * pq.dsub] for c in chunks]).contiguous()
        elif _is_device_tensor(x):
            assert x.dim() == 2 and x.shape[1] == self._d, "dimension mismatch"
            n = int(x.shape[0])

            def piece(m):
                return x[:, m * pq.dsub:(m + 1) * pq.dsub].contiguous()
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 2 and x.shape[1] == self._d, "dimension mismatch"
            n = int(x.shape[0])

            def piece(m):
                return np.ascontiguousarray(x[:, m * pq.dsub:(m + 1) * pq.dsub])
        if n < pq.ksub:
            raise RuntimeError(f"IndexPQ.train: {n} training rows, fewer than the {pq.ksub} centroids of a sub-quantizer")
        cents = np.empty((pq.M, pq.ksub, pq.dsub), dtype=np.float32)
        for m in range(pq.M):
            km = Kmeans(pq.dsub, pq.ksub, niter=pq.niter, seed=pq.seed, device=self.device)
            km.train(piece(m))
            cents[m] = km.centroids
        pq.centroids = cents

    def get_codes(self, i0: int = 0, n: int = -1) -> np.ndarray:
        """The codes of the rows ``[i0, i0 + n)`` as numpy ``(n, M)`` uint8 (n = -1: to the end)."""
        i0 = int(i0)
        n = self.ntotal - i0 if int(n) < 0 else int(n)
        out = np.empty((n, self.pq.M), dtype=np.uint8)
        self._bind_stream(False)
        self._check(self._fn("get_codes")(self._h, i0, n, ctypes.c_void_p(out.ctypes.data), _lib.MEM_HOST))
        return out

    @property
    def codes(self) -> np.ndarray:
        """faiss's ``index.codes``: every row's code, ``(ntotal, M)`` uint8."""
        return self.get_codes()

    last_pq_plan = _CodeIndex._last_plan


# ---------------------------------------------------------------------------
# faiss.IndexIVFScalarQuantizer (include/fx_index.h "inverted file over 8-bit codes")
# ---------------------------------------------------------------------------
class IndexIVFScalarQuantizer(IndexIVFFlat):
    """``faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric,
    by_residual)`` with 8-bit codes: ``IndexIVFFlat``'s lists holding
    ``IndexScalarQuantizer``'s rows, one byte per dimension.  With
    ``by_residual`` (faiss's default) a row of list l is encoded as ``x -
    c_l`` and decodes to ``c_l + decode(code)``, so the quantiser's box is the
    size of a cluster, not of the corpus.  A search ranks the DECODED rows of
    the probed lists exactly: ids bit-exact, distances the fp64 sum rounded
    once, ranked by (distance, list number, insertion order within the list).

    The definition restates faiss's from memory and is not checked against a
    faiss build; in particular faiss ranks a row by the distance between the
    query's residual and the decoded residual, this class by the decoded row.

    ``train(x)`` trains the coarse quantizer as ``IndexIVFFlat.train`` does if
    it is untrained, then the quantiser's tables on the residuals of ``x``.

    Not offered: the other qtypes, selectors, ``remove_ids``,
    ``range_search``, ``reconstruct*``, ``write_index`` / ``read_index``."""

    _PFX = "fx_ivfsq_"

    def __init__(self, quantizer, d: int, nlist: int, qtype: int = ScalarQuantizer.QT_8bit,
                 metric: int = METRIC_L2, by_residual: bool = True, device: int = 0, niter: int = 10,
                 seed: int = 1234):
        qtype = int(qtype)
        if qtype not in (ScalarQuantizer.QT_8bit, ScalarQuantizer.QT_8bit_uniform):
            name = _QT_NAMES.get(qtype, f"qtype {qtype}")
            raise NotImplementedError(f"IndexIVFScalarQuantizer: {name} is not offered (QT_8bit, QT_8bit_uniform)")
        assert isinstance(quantizer, _FlatIndex), "quantizer must be an IndexFlatL2 / IndexFlatIP of this module"
        assert quantizer.d == int(d), f"quantizer has d = {quantizer.d}, the index d = {int(d)}"
        assert quantizer.device == int(device), f"quantizer on cuda:{quantizer.device}, index on cuda:{int(device)}"
        assert metric in (METRIC_L2, METRIC_INNER_PRODUCT), "metric must be METRIC_L2 or METRIC_INNER_PRODUCT"
        self.quantizer = quantizer
        self._lib = quantizer._lib
        self._d, self.nlist, self.metric_type = int(d), int(nlist), int(metric)
        self.qtype, self.by_residual = qtype, bool(by_residual)
        self.storage_dtype, self.device = "int8", int(device)
        self.nprobe = 1
        self.niter, self.seed = int(niter), int(seed)
        self.verbose = False
        self._mode = None
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(quantizer._h, self._d, self.nlist, qtype, self.metric_type,
                                       1 if self.by_residual else 0, ctypes.byref(self._h)))

    @property
    def code_size(self) -> int:
        return self._d

    @property
    def is_trained(self) -> bool:
        if self.quantizer.ntotal != self.nlist:
            return False
        v = ctypes.c_int(0)
        self._check(self._fn("is_trained")(self._h, ctypes.byref(v)))
        return bool(v.value)

    _rows = _rows

    def train(self, x) -> None:
        """k-means on the quantizer if it holds no centroids yet (as
        ``IndexIVFFlat.train``), then per-dimension (``QT_8bit_uniform``:
        global) min and max of the residuals of ``x``: numpy rows, a device
        tensor, or a flat index of this module (its stored rows, gathered on
        the device chunk by chunk).  A no-op on a trained index, as faiss."""
        if self.is_trained:
            return
        assert self.ntotal == 0, "train on an index that holds rows: reset() it first"
        if self.quantizer.ntotal != self.nlist:
            IndexIVFFlat.train(self, x)
        if _is_index(x):
            flat = _flat(x)
            assert not flat.has_ids and flat.device == self.device and flat.d == self._d
            t = _torch()
            n = flat.ntotal
            for r0 in range(0, n, KMEANS_CHUNK):
                keys = t.arange(r0, min(n, r0 + KMEANS_CHUNK), dtype=t.int64, device=t.device("cuda", self.device))
                ptr, code, mem, nr, _keep = self._rows(flat.reconstruct_batch(keys + flat._id_offset, dtype="storage"))
                self._check(self._fn("train")(self._h, nr, ptr, code, mem, 1))
            self._check(self._fn("train")(self._h, 0, None, _lib.F32, _lib.MEM_DEVICE, 0))
            return
        ptr, code, mem, n, _keep = self._rows(x)
        self._check(self._fn("train")(self._h, n, ptr, code, mem, 0))

    @property
    def trained(self) -> np.ndarray:
        """faiss's ``sq.trained``: ``[vmin[d] | vdiff[d]]`` fp32 (``QT_8bit_uniform``:
        ``[vmin, vdiff]``), of the residuals with ``by_residual``."""
        out = np.empty(2 * self._d, dtype=np.float32)
        self._check(self._fn("get_trained")(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        if self.qtype == ScalarQuantizer.QT_8bit_uniform:
            return np.array([out[0], out[self._d]], dtype=np.float32)
        return out

    def set_trained(self, arr) -> None:
        """Install tables kept with numpy (the array ``trained`` returned); the
        quantizer must hold its centroids already."""
        assert self.ntotal == 0, "set_trained on an index that holds rows: reset() it first"
        assert self.quantizer.ntotal == self.nlist, "the quantizer is not trained"
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        if self.qtype == ScalarQuantizer.QT_8bit_uniform and a.size == 2:
            a = np.concatenate([np.full(self._d, a[0], np.float32), np.full(self._d, a[1], np.float32)])
        assert a.size == 2 * self._d, f"trained must hold {2 * self._d} floats"
        self._check(self._fn("set_trained")(self._h, a.ctypes.data_as(ctypes.c_void_p)))

    def get_list_codes(self, l: int) -> np.ndarray:
        """The codes of list ``l`` in insertion order: faiss's unsigned bytes
        ``(n, d)`` uint8."""
        n = ctypes.c_int64(0)
        self._check(self._fn("list_codes")(self._h, int(l), None, 0, ctypes.byref(n)))
        out = np.empty((n.value, self._d), dtype=np.uint8)
        if n.value:
            self._check(self._fn("list_codes")(self._h, int(l), out.ctypes.data_as(ctypes.c_void_p), n.value,
                                               ctypes.byref(n)))
        return out


# ---------------------------------------------------------------------------
# faiss.IndexIVFPQ (include/fx_index.h "inverted file over product-quantized codes")
# ---------------------------------------------------------------------------
class IndexIVFPQ(IndexIVFFlat):
    """``faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits, metric)`` with 8-bit
    codes: ``IndexIVFFlat``'s lists holding ``IndexPQ``'s rows, M bytes each.
    With ``by_residual`` (faiss's default) a row of list l is encoded as ``x -
    c_l`` and decodes to ``c_l + decode(code)``, so the codebook covers a
    cluster, not the corpus.  A search ranks the DECODED rows of the probed
    lists exactly: ids bit-exact, distances the fp64 sum rounded once, ranked
    by (distance, list number, insertion order within the list).

    The definition restates faiss's from memory and is not checked against a
    faiss build; in particular faiss ranks a row by the distance between the
    query's residual and the decoded residual, this class by the decoded row.

    ``pq`` is the ``ProductQuantizer`` view of the codebook (``pq.centroids``
    get and set).  ``train(x)`` trains the coarse quantizer as
    ``IndexIVFFlat.train`` does if it is untrained, then M times ``Kmeans(dsub,
    256, niter=pq_niter, seed)`` on the slices of the residuals of ``x``.

    Not offered: ``nbits != 8`` (``NotImplementedError``), precomputed tables,
    polysemous search, OPQ, fast-scan, selectors, ``remove_ids``,
    ``range_search``, ``reconstruct*``, ``write_index`` / ``read_index``."""

    _PFX = "fx_ivfpq_"

    def __init__(self, quantizer, d: int, nlist: int, M: int, nbits: int = 8, metric: int = METRIC_L2,
                 by_residual: bool = True, device: int = 0, niter: int = 10, seed: int = 1234, pq_niter: int = 25):
        d, M, nbits = int(d), int(M), int(nbits)
        if nbits != 8:
            raise NotImplementedError(f"IndexIVFPQ: nbits = {nbits} is not offered (8)")
        if d <= 0 or M <= 0 or d % M != 0:
            raise ValueError(f"IndexIVFPQ: d = {d} is not a multiple of M = {M}")
        assert isinstance(quantizer, _FlatIndex), "quantizer must be an IndexFlatL2 / IndexFlatIP of this module"
        assert quantizer.d == d, f"quantizer has d = {quantizer.d}, the index d = {d}"
        assert quantizer.device == int(device), f"quantizer on cuda:{quantizer.device}, index on cuda:{int(device)}"
        assert metric in (METRIC_L2, METRIC_INNER_PRODUCT), "metric must be METRIC_L2 or METRIC_INNER_PRODUCT"
        self.quantizer = quantizer
        self._lib = quantizer._lib
        self._d, self.nlist, self.metric_type = d, int(nlist), int(metric)
        self.by_residual = bool(by_residual)
        self.storage_dtype, self.device = "uint8", int(device)
        self.nprobe = 1
        self.niter, self.seed = int(niter), int(seed)
        self.verbose = False
        self._mode = None
        self.pq = ProductQuantizer(self, d, M, nbits, pq_niter, seed)
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(quantizer._h, d, self.nlist, M, nbits, self.metric_type,
                                       1 if self.by_residual else 0, ctypes.byref(self._h)))

    @property
    def code_size(self) -> int:
        return self.pq.M

    @property
    def is_trained(self) -> bool:
        if self.quantizer.ntotal != self.nlist:
            return False
        v = ctypes.c_int(0)
        self._check(self._fn("is_trained")(self._h, ctypes.byref(v)))
        return bool(v.value)

    _rows = _rows

    def _residuals(self, x):
        """A device tensor ``[n][d]`` fp32 of the residuals of the rows ``x``
        (numpy or a device tensor), through ``fx_ivfpq_residuals``."""
        t = _torch()
        ptr, code, mem, n, _keep = self._rows(x)
        self._bind_stream(True)  # (the output is a tensor of the current stream)
        out = t.empty((n, self._d), dtype=t.float32, device=t.device("cuda", self.device))
        self._check(self._fn("residuals")(self._h, n, ptr, code, mem, ctypes.c_void_p(out.data_ptr()), _lib.MEM_DEVICE))
        return out

    def train(self, x) -> None:
        """k-means on the quantizer if it holds no centroids yet (as
        ``IndexIVFFlat.train``), then the codebook: the residuals of ``x``
        (numpy rows, a device tensor, or a flat index of this module, its
        stored rows gathered chunk by chunk) are computed on the device, and
        ``Kmeans(dsub, 256, niter=pq.niter, seed=pq.seed)`` runs on the slice
        of every sub-quantizer; the centroids are installed as
        ``pq.centroids``.  A no-op on a trained index, as faiss.  Fewer than
        256 rows is an error."""
        if self.is_trained:
            return
        assert self.ntotal == 0, "train on an index that holds rows: reset() it first"
        if self.quantizer.ntotal != self.nlist:
            IndexIVFFlat.train(self, x)
        t = _torch()
        pq = self.pq
        flat = _flat(x) if _is_index(x) else None
        if flat is not None:
            assert not flat.has_ids and flat.device == self.device and flat.d == self._d
        n = flat.ntotal if flat is not None else int(x.shape[0])
        if n < pq.ksub:
            raise RuntimeError(f"IndexIVFPQ.train: {n} training rows, fewer than the {pq.ksub} centroids of a "
                               f"sub-quantizer")
        chunks = []
        for r0 in range(0, n, KMEANS_CHUNK):
            if flat is not None:
                keys = t.arange(r0, min(n, r0 + KMEANS_CHUNK), dtype=t.int64, device=t.device("cuda", self.device))
                chunks.append(self._residuals(flat.reconstruct_batch(keys + flat._id_offset, dtype="storage")))
            else:
                chunks.append(self._residuals(x[r0:r0 + KMEANS_CHUNK]))
        cents = np.empty((pq.M, pq.ksub, pq.dsub), dtype=np.float32)
        for m in range(pq.M):
            km = Kmeans(pq.dsub, pq.ksub, niter=pq.niter, seed=pq.seed, device=self.device)
            km.train(t.cat([c[:, m * pq.dsub:(m + 1) * pq.dsub] for c in chunks]).contiguous())
            cents[m] = km.centroids
        pq.centroids = cents

    def get_list_codes(self, l: int) -> np.ndarray:
        """The codes of list ``l`` in insertion order: ``(n, M)`` uint8."""
        n = ctypes.c_int64(0)
        self._check(self._fn("list_codes")(self._h, int(l), None, 0, ctypes.byref(n)))
        out = np.empty((n.value, self.pq.M), dtype=np.uint8)
        if n.value:
            self._check(self._fn("list_codes")(self._h, int(l), out.ctypes.data_as(ctypes.c_void_p), n.value,
                                               ctypes.byref(n)))
        return out


def write_index(index, path: str) -> None:
    """``faiss.write_index`` (faiss_store.py:91): IxF2 file, fp32 codes; a
    labelled index (``IndexIDMap`` / ``IndexIDMap2``) as an IxM2 file."""
    if isinstance(index, IndexIVFPQ):
        raise NotImplementedError("write_index of an IndexIVFPQ: write its quantizer, keep `pq.centroids` with numpy "
                                  "and re-add the rows")
    if isinstance(index, IndexIVFScalarQuantizer):
        raise NotImplementedError("write_index of an IndexIVFScalarQuantizer: write its quantizer, keep `trained` "
                                  "with numpy and re-add the rows")
    if isinstance(index, IndexIVFFlat):
        raise NotImplementedError("write_index of an IndexIVFFlat: write its quantizer and re-add the rows")
    if isinstance(index, IndexScalarQuantizer):
        raise NotImplementedError("write_index of an IndexScalarQuantizer: keep `trained` with numpy and re-add the rows")
    if isinstance(index, IndexPQ):
        raise NotImplementedError("write_index of an IndexPQ: keep `pq.centroids` with numpy and re-add the rows")
    index = _flat(index)
    check(index._lib.fx_index_write(index._h, str(path).encode()), index._lib)


def read_index(path: str, dtype: str = "float32", device: int = 0):
    """``faiss.read_index`` (faiss_store.py:106): IxF2 file -> HBM
    ``IndexFlatL2``; an IxMp / IxM2 file -> ``IndexIDMap2`` around one."""
    h = ctypes.c_void_p()
    rc = lib.fx_index_read(str(path).encode(), _DTYPES[dtype], int(device), ctypes.byref(h))
    check(rc)
    flat = IndexFlatL2(0, dtype=dtype, device=device, _handle=h)
    return IndexIDMap2._wrap(flat) if flat.has_ids else flat


def synth_fill(out, row0: int, seed: int) -> None:
    """Fill a 2-D device tensor with rows ``row0..`` of the synthetic corpus
    (definition shared with oracle/flat_l2.py ``synth``)."""
    t = _torch()
    assert _is_device_tensor(out) and out.dim() == 2 and out.is_contiguous()
    s = t.cuda.current_stream(out.device).cuda_stream
    check(lib.fx_synth_fill(ctypes.c_void_p(out.data_ptr()), int(row0), out.shape[0], out.shape[1],
                            _tensor_dtype(out), int(seed), out.device.index, ctypes.c_void_p(s)))


def merge_shards(metric: int, Dg, Ig, k: int, D_out=None, I_out=None):
    """Merge gathered per-shard results ``Dg``/``Ig`` shaped (G, nq, k) (device
    tensors) into the global top-k (the step after the RCCL allgather)."""
    t = _torch()
    G, nq, kk = Dg.shape
    assert kk == k and Ig.shape == Dg.shape
    if D_out is None:
        D_out = t.empty((nq, k), dtype=t.float32, device=Dg.device)
    if I_out is None:
        I_out = t.empty((nq, k), dtype=t.int64, device=Dg.device)
    s = t.cuda.current_stream(Dg.device).cuda_stream
    check(lib.fx_merge_shards(int(metric), G, nq, k, ctypes.c_void_p(Dg.data_ptr()), ctypes.c_void_p(Ig.data_ptr()),
                              ctypes.c_void_p(D_out.data_ptr()), ctypes.c_void_p(I_out.data_ptr()),
                              Dg.device.index, ctypes.c_void_p(s)))
    return D_out, I_out
