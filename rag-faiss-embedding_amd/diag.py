"""Indexes bound to the diagnostic build of the library (tests only).

``libfx_index_diag.so`` is ``libfx_index.so``'s kernels with the host side
compiled under ``-DFX_DIAG`` (``make -C csrc diag``): its option table adds
the test hooks the product library does not carry -- ``force_fallback``
(1: every query through the device-gated re-scan, 2: through the exact fp64
scan) and ``scan_dbg`` 32 (the scan's whole key matrix dumped to
``FX_SCAN_KEYS``) -- plus the FX_SCAN_TRACE / _CAND dumps, and the dumps of
the newer scans' lists, written per pass before the refine reads them and the
exact path writes over them (paths read when the index is created):

``FX_SQ_CAND``   fx_sq_search: ``cand_d``, ``cand_i`` [qtiles][splits][128][KP],
                 ``sigma`` [nq_pad], ``E`` [nq], the shift [nq] f64, the digit
                 planes [3][nq_pad][row_bytes] i8, the index words [4] u32
                 (max n_c, max sum c'^2, rho_dec as float bits, 0) and the
                 rows' ``n_c`` [ntotal] (tests/test_sq_scan_parity.py)
``FX_IVF_CAND``  fx_ivf_search: ``cand_d``, ``cand_i`` [nq][slots][KP], the
                 probed lists [nq][nprobe] i64, ``list_off`` [nlist + 1] i32
                 (tests/test_ivf_scan_parity.py)
``FX_IVFSQ_CAND``  fx_ivfsq_search: ``cand_d``, ``cand_i`` [nq][slots][KP], the
                 probed lists [nq][nprobe] i64, ``list_off`` [nlist + 1] i32, the
                 pairs' ``sigma``, shift and ``E`` [pairs_pad] f32 each, the digit
                 planes [3][pairs_pad][row_bytes] i8 and the rows' ``n_c``
                 [ntotal] (tests/test_ivfsq_scan_parity.py)
``FX_PQ_CAND``   fx_pq_search: ``cand_d``, ``cand_i`` [qtiles][splits][128][KP],
                 ``E`` [nq], the shift [nq] f64, the query planes [2][nq_pad][kp]
                 bf16 ([hi | lo]), the rows' codes [ntotal][roundup(M, 16)] u8 and
                 ``n_y`` [ntotal] (tests/test_pq_scan_parity.py)
``FX_IVFPQ_CAND``  fx_ivfpq_search: ``cand_d``, ``cand_i`` [nq][slots][KP], the
                 probed lists [nq][nprobe] i64, ``list_off`` [nlist + 1] i32, the
                 pairs' shift and ``E`` [pairs_pad] f32 each, the operand planes
                 [2][op_rows][kp] bf16 ([hi | lo]; op_rows = pairs_pad for L2 with
                 by_residual, else roundup(nq, 128)), the rows' codes
                 [ntotal][roundup(M, 16)] u8 and ``n_y`` [ntotal]
                 (tests/test_ivfpq_scan_parity.py)

The classes here are the faiss.py ones with every call going to that build.
"""
from __future__ import annotations

import ctypes

from . import _lib
from . import faiss as _faiss

if not _lib.DIAG_PATH.exists():
    raise ImportError(f"{_lib.DIAG_PATH} not found: build it with `make -C {_lib._HERE / 'csrc'} diag`")

lib = _lib.bind(_lib.DIAG_PATH)


class IndexFlatL2(_faiss.IndexFlatL2):
    _lib = lib


class IndexFlatIP(_faiss.IndexFlatIP):
    _lib = lib


class IndexScalarQuantizer(_faiss.IndexScalarQuantizer):
    """``force_fallback`` comes from ``FX_FORCE_FALLBACK`` in the environment
    when the index is created (it has no option table of its own)."""

    _lib = lib


class IndexPQ(_faiss.IndexPQ):
    """``FX_PQ_CAND`` and ``FX_FORCE_FALLBACK`` come from the environment when
    the index is created."""

    _lib = lib


class IndexIVFFlat(_faiss.IndexIVFFlat):
    """An inverted file lives in the build of its quantizer: this one takes a
    quantizer of this module.  ``FX_IVF_CAND`` comes from the environment when
    the index is created; ``force_fallback`` is the quantizer's option."""

    def __init__(self, quantizer, *args, **kwargs):
        assert quantizer._lib is lib, "the quantizer must be an index of the diagnostic build"
        super().__init__(quantizer, *args, **kwargs)


class IndexIVFScalarQuantizer(_faiss.IndexIVFScalarQuantizer):
    """As ``IndexIVFFlat`` above: a quantizer of this module.  ``FX_IVFSQ_CAND``
    and ``FX_FORCE_FALLBACK`` come from the environment when the index is
    created."""

    def __init__(self, quantizer, *args, **kwargs):
        assert quantizer._lib is lib, "the quantizer must be an index of the diagnostic build"
        super().__init__(quantizer, *args, **kwargs)


class IndexIVFPQ(_faiss.IndexIVFPQ):
    """As ``IndexIVFFlat`` above: a quantizer of this module.  ``FX_IVFPQ_CAND``
    and ``FX_FORCE_FALLBACK`` come from the environment when the index is
    created."""

    def __init__(self, quantizer, *args, **kwargs):
        assert quantizer._lib is lib, "the quantizer must be an index of the diagnostic build"
        super().__init__(quantizer, *args, **kwargs)


def read_index(path: str, dtype: str = "float32", device: int = 0) -> IndexFlatL2:
    h = ctypes.c_void_p()
    _lib.check(lib.fx_index_read(str(path).encode(), _faiss._DTYPES[dtype], int(device), ctypes.byref(h)), lib)
    return IndexFlatL2(0, dtype=dtype, device=device, _handle=h)
