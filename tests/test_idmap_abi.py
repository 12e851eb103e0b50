"""CPU checks of the stable-id ABI (include/fx_index.h "stable ids"): the header
declares and documents the four calls with their faiss counterparts, the
library exports them, the ctypes table binds them, their argument checks run
without a device, and the reader's parser accepts the IxM2 / IxMp layout built
by hand here (and rejects its damaged headers) before it ever needs a GPU."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
NEW = ("fx_index_add_with_ids", "fx_index_has_ids", "fx_index_get_ids", "fx_index_rows_of_ids")


def test_header_declares_the_four_calls():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ws = r"\s*"
    assert re.search(r"int\s+fx_index_add_with_ids\s*\(" + ws.join(
        [r"FxIndex\s*\*\s*index\s*,", r"int64_t\s+n\s*,", r"const\s+void\s*\*\s*x\s*,", r"int\s+x_dtype\s*,",
         r"int\s+x_mem\s*,", r"const\s+int64_t\s*\*\s*ids\s*,", r"int\s+ids_mem\s*\)\s*;"]), code)
    assert re.search(r"int\s+fx_index_has_ids\s*\(\s*const\s+FxIndex\s*\*\s*index\s*,\s*int\s*\*\s*out\s*\)\s*;", code)
    assert re.search(r"int\s+fx_index_get_ids\s*\(\s*FxIndex\s*\*\s*index\s*,\s*int64_t\s+i0\s*,\s*int64_t\s+n\s*,"
                     r"\s*int64_t\s*\*\s*out\s*,\s*int\s+out_mem\s*\)\s*;", code)
    assert re.search(r"int\s+fx_index_rows_of_ids\s*\(\s*FxIndex\s*\*\s*index\s*,\s*const\s+int64_t\s*\*\s*ids\s*,"
                     r"\s*int64_t\s+n\s*,\s*int\s+ids_mem\s*,\s*int64_t\s*\*\s*rows\s*,\s*int\s+rows_mem\s*\)\s*;", code)


def test_header_names_the_faiss_counterparts_and_the_mode():
    text = HEADER.read_text()
    for name in ("faiss_Index_add_with_ids", "faiss_IndexIDMap_id_map", "faiss_IndexIDMap2_new", "IxM2", "IxMp",
                 "stable ids"):
        assert name in text, name
    # -1 is documented as indistinguishable from the missing marker; the file layout as unchecked against faiss
    assert re.search(r"-1 is legal\s+\*?\s*too but cannot be told from", text)
    assert "not checked against a faiss build" in text


def test_library_exports_and_binds_the_calls():
    for name in NEW:
        assert hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i
        assert getattr(_lib.lib, name).argtypes == args
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [7, 2, 5, 6]


def test_null_and_negative_arguments_without_device():
    lib = _lib.lib
    x = (ctypes.c_float * 4)()
    ids = (ctypes.c_int64 * 1)(5)
    out = ctypes.c_int(0)
    assert lib.fx_index_add_with_ids(None, 1, x, 0, 0, ids, 0) == -1
    assert "null" in _lib.last_error()
    assert lib.fx_index_add_with_ids(None, -1, x, 0, 0, ids, 0) == -1
    assert lib.fx_index_has_ids(None, ctypes.byref(out)) == -1
    assert lib.fx_index_get_ids(None, 0, 1, ids, 0) == -1
    assert lib.fx_index_get_ids(None, 0, -1, ids, 0) == -1
    assert lib.fx_index_rows_of_ids(None, ids, 1, 0, ids, 0) == -1
    assert lib.fx_index_rows_of_ids(None, ids, -1, 0, ids, 0) == -1


# ---- the IxM2 byte layout, built by hand ---------------------------------------
def header_fields(d, nt, metric=1):
    """i32 d, i64 ntotal, i64 1<<20, i64 1<<20, u8 is_trained, i32 metric."""
    return struct.pack("<iqqqBi", d, nt, 1 << 20, 1 << 20, 1, metric)


def ixf2(rows):
    nt, d = rows.shape
    return b"IxF2" + header_fields(d, nt) + struct.pack("<q", nt * d) + rows.astype("<f4").tobytes()


def ixm2(rows, labels, fourcc=b"IxM2"):
    nt, d = rows.shape
    return fourcc + header_fields(d, nt) + ixf2(rows) + struct.pack("<q", len(labels)) + \
        np.asarray(labels, dtype="<i8").tobytes()


def read(path, data):
    path.write_bytes(data)
    h = ctypes.c_void_p()
    rc = _lib.lib.fx_index_read(str(path).encode(), 0, 0, ctypes.byref(h))
    return rc, h


def test_reader_parses_the_ixm2_layout(tmp_path):
    """Without a GPU a well-formed file gets through the parser to the index
    creation (FX_E_HIP -2, not FX_E_IO -3); with one it reads back labelled."""
    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    labels = np.array([-7, (1 << 40) + 1, -7], dtype=np.int64)
    assert len(header_fields(4, 3)) == 33 and len(ixf2(rows)) == 4 + 33 + 8 + 48
    have_gpu = _lib.device_count() > 0
    for fourcc in (b"IxM2", b"IxMp"):
        rc, h = read(tmp_path / "a.index", ixm2(rows, labels, fourcc))
        assert rc == (0 if have_gpu else -2), _lib.last_error()
        if rc == 0:
            has = ctypes.c_int(0)
            assert _lib.lib.fx_index_has_ids(h, ctypes.byref(has)) == 0 and has.value == 1
            got = np.zeros(3, dtype=np.int64)
            assert _lib.lib.fx_index_get_ids(h, 0, 3, got.ctypes.data_as(ctypes.c_void_p), 0) == 0
            assert got.tolist() == labels.tolist()
            _lib.lib.fx_index_free(h)
    rc, h = read(tmp_path / "b.index", ixf2(rows))
    assert rc == (0 if have_gpu else -2)
    if rc == 0:
        has = ctypes.c_int(1)
        assert _lib.lib.fx_index_has_ids(h, ctypes.byref(has)) == 0 and has.value == 0
        _lib.lib.fx_index_free(h)


def test_reader_rejects_damaged_ixm2_headers(tmp_path):
    rows = np.ones((3, 4), dtype=np.float32)
    good = ixm2(rows, [1, 2, 3])
    # cut anywhere inside the two headers (the sub-index's ends at byte 82)
    for cut in (0, 3, 4, 20, 36, 37, 40, 41, 60, 77, 81):
        rc, h = read(tmp_path / "cut.index", good[:cut])
        assert rc == -3 and not h.value, cut
    # a foreign fourcc outside or inside; a wrapper that disagrees with its sub-index
    for bad in (b"XxF2" + good[4:], good[:37] + b"XxF2" + good[41:], good[:37] + b"IxM2" + good[41:],
                b"IxM2" + header_fields(4, 2) + good[37:], b"IxM2" + header_fields(8, 3) + good[37:]):
        rc, h = read(tmp_path / "bad.index", bad)
        assert rc == -3 and not h.value
        assert _lib.last_error()


@pytest.mark.parametrize("n_ids", [2, 4])
def test_id_count_must_match_the_rows(tmp_path, n_ids):
    """i64 n of the id map differing from ntotal: FX_E_IO once a device lets the
    reader get that far (FX_E_HIP before that without one)."""
    rows = np.ones((3, 4), dtype=np.float32)
    rc, h = read(tmp_path / "n.index", ixm2(rows, list(range(n_ids))))
    assert rc == (-3 if _lib.device_count() > 0 else -2) and not h.value
