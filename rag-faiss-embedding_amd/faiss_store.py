"""``FAISSVectorStore`` on the MI355X flat index.

Same class, methods, attributes and error behaviour as the reference
``faiss_store.py:10-128``; only the engine underneath changes (the HIP index
of :mod:`.faiss` instead of faiss-cpu).  Logging uses the stdlib instead of
loguru.  The mapping sidecar is read without unpickling (:mod:`._mapping`).

Extensions (keyword-only, defaults reproduce the reference): ``dtype`` of the
HBM codes ("float32" like the reference, or "bfloat16"/"float16") and the
GPU ``device``.  ``add_vectors``/``search`` also accept torch tensors that
already live on the GPU (encoder hand-off without ``.cpu().numpy()``).
``remove_vectors(ids)`` deletes documents' rows in place (the reference can
only rebuild the whole index).
"""
from __future__ import annotations

import logging
import os
from typing import List, Optional, Tuple

import numpy as np

from . import _mapping
from . import faiss as _fx

logger = logging.getLogger("rag_faiss_embedding_amd.faiss_store")


class FAISSVectorStore:
    """One store per process (faiss_store.py:14-17): later constructions
    return the first instance and ignore their arguments (:21-22)."""

    _instance = None
    _initialized = False
    ivf = None  # the IndexIVFFlat / IndexIVFScalarQuantizer / IndexIVFPQ over the store's rows (build_ivf); dropped by every
                # call that changes the rows
    sq = None   # the IndexScalarQuantizer over the store's rows (build_sq); dropped by the same calls
    pq = None   # the IndexPQ over the store's rows (build_pq); dropped by the same calls

    def __new__(cls, *args, **kwargs):
        if cls._instance is None:
            cls._instance = super().__new__(cls)
        return cls._instance

    def __init__(self, dimension: int = 384, index_path: str = "data/faiss_index.bin", *,
                 dtype: str = "float32", device: int = 0):
        if self._initialized:
            return
        self.dimension, self.index_path = dimension, index_path
        self.dtype, self.device = dtype, device
        self.doc_ids: List[int] = []
        self.index = _fx.IndexFlatL2(dimension, dtype=dtype, device=device)
        if os.path.exists(index_path):
            self.load_index()
        logger.info("store ready: d=%d, %s on cuda:%d", dimension, dtype, device)
        self._initialized = True

    @staticmethod
    def _as_rows(x):
        """list -> float32 array; a single vector -> one row (:38-42)."""
        if isinstance(x, list):
            x = np.array(x, dtype=np.float32)
        return x.reshape(1, -1) if len(x.shape) == 1 else x

    def add_vectors(self, vectors, ids: List[int]):
        """faiss_store.py:36-47.  The ids are recorded before the rows go in,
        and their count is not checked against the rows (as there)."""
        rows = self._as_rows(vectors)
        self.ivf = self.sq = self.pq = None
        self.doc_ids.extend(ids)
        self.index.add(rows)
        logger.info("add: %d ids -> ntotal %d", len(ids), self.index.ntotal)

    def _rows_selector(self, allowed_ids):
        """Document ids -> the index rows that carry them (every row of an id
        that occurs more than once in ``doc_ids``; unknown ids select nothing)
        as ``SearchParameters`` with an ``IDSelectorBatch``."""
        allowed = set(int(a) for a in allowed_ids)
        rows = [r for r, doc in enumerate(self.doc_ids) if doc in allowed]
        return _fx.SearchParameters(sel=_fx.IDSelectorBatch(np.asarray(rows, dtype=np.int64)))

    def build_ivf(self, nlist: int, nprobe: int = 8, qtype=None, pq_m=None):
        """An ``IndexIVFFlat`` over the store's rows (extension): the coarse
        quantizer is trained on the store's own index, so the rows never leave
        the GPU, and the rows are added with ids equal to their row numbers, so
        ``doc_ids`` keeps mapping results.  Kept as ``self.ivf`` until a call
        changes the rows; ``search(..., nprobe=n)`` uses it.  With a ``qtype``
        (``ScalarQuantizer.QT_8bit`` / ``QT_8bit_uniform``) the lists hold one
        byte per dimension instead: an ``IndexIVFScalarQuantizer`` with
        residual encoding, searched the same way (the k nearest DECODED rows
        of the probed lists).  With ``pq_m = M`` the lists hold M bytes per
        row: an ``IndexIVFPQ`` with residual encoding, trained on the store's
        rows and searched the same way.  ``qtype`` and ``pq_m`` together are a
        ``ValueError``.  Errors are logged and raised again, as in
        ``load_index``."""
        if qtype is not None and pq_m is not None:
            raise ValueError("build_ivf: qtype and pq_m name two different list encodings; pass one")
        try:
            quantizer = _fx.IndexFlatL2(self.dimension, device=self.device)
            if pq_m is not None:
                ivf = _fx.IndexIVFPQ(quantizer, self.dimension, int(nlist), int(pq_m), 8, _fx.METRIC_L2,
                                     device=self.device)
            elif qtype is None:
                ivf = _fx.IndexIVFFlat(quantizer, self.dimension, int(nlist), _fx.METRIC_L2, dtype=self.dtype,
                                       device=self.device)
            else:
                ivf = _fx.IndexIVFScalarQuantizer(quantizer, self.dimension, int(nlist), qtype, _fx.METRIC_L2,
                                                  device=self.device)
            ivf.nprobe = int(nprobe)
            ivf.train(self.index)
            ivf.add_from_index(self.index)
            n = self.index.ntotal
            self.ivf = ivf
            logger.info("build_ivf: %d rows in %d lists, nprobe %d", n, nlist, nprobe)
            return ivf
        except Exception as e:
            logger.error("build_ivf failed: %s", e)
            raise

    def build_sq(self, qtype: int = _fx.ScalarQuantizer.QT_8bit):
        """An ``IndexScalarQuantizer`` over the store's rows (extension): one
        byte per dimension, trained on and filled from the store's own index
        on the device.  Ids are row numbers, so ``doc_ids`` keeps mapping
        results.  Kept as ``self.sq`` until a call changes the rows;
        ``search(..., sq=True)`` uses it.  Errors are logged and raised again,
        as in ``load_index``."""
        try:
            sq = _fx.IndexScalarQuantizer(self.dimension, qtype, _fx.METRIC_L2, device=self.device)
            sq.train(self.index)
            sq.add_from_index(self.index)
            self.sq = sq
            logger.info("build_sq: %d rows, %d bytes per row", self.index.ntotal, sq.code_size)
            return sq
        except Exception as e:
            logger.error("build_sq failed: %s", e)
            raise

    def build_pq(self, M: int):
        """An ``IndexPQ`` over the store's rows (extension): ``M`` bytes per
        row, trained on and filled from the store's own index on the device.
        Ids are row numbers, so ``doc_ids`` keeps mapping results.  Kept as
        ``self.pq`` until a call changes the rows; ``search(..., pq=True)``
        uses it.  Errors are logged and raised again, as in ``load_index``."""
        try:
            pq = _fx.IndexPQ(self.dimension, M, 8, _fx.METRIC_L2, device=self.device)
            pq.train(self.index)
            pq.add_from_index(self.index)
            self.pq = pq
            logger.info("build_pq: %d rows, %d bytes per row", self.index.ntotal, pq.code_size)
            return pq
        except Exception as e:
            logger.error("build_pq failed: %s", e)
            raise

    def search(self, query_vector, k: int = 5, allowed_ids=None, nprobe=None, sq: bool = False, pq: bool = False
               ) -> Tuple[np.ndarray, List[int]]:
        """faiss_store.py:49-81: one query; index rows map to document ids,
        -1 and rows past the id list are dropped; on any error the result is
        ``(np.array([]), [])``.  Any k, as faiss (k > ``FX_MAX_K`` = 1024
        takes the index's exact sort path).

        ``allowed_ids`` (document ids; extension): only those documents are
        ranked -- the index's filtered search over their rows (k <=
        ``FX_MAX_K``), so a narrow filter still returns its k nearest.

        ``nprobe`` (extension): search the ``IndexIVFFlat`` of ``build_ivf``
        over that many lists instead of the whole index (no ``allowed_ids``,
        k <= ``FX_MAX_K``); without a built one the call fails as any other
        error here does.

        ``sq=True`` (extension): search the ``IndexScalarQuantizer`` of
        ``build_sq`` -- the k nearest DECODED rows (no ``allowed_ids``, no
        ``nprobe``, k <= ``FX_MAX_K``).

        ``pq=True`` (extension): the same over the ``IndexPQ`` of ``build_pq``."""
        try:
            q = query_vector
            if isinstance(q, list):
                q = np.array(q, dtype=np.float32)
            if pq:
                if self.pq is None:
                    raise RuntimeError("search(pq=True) needs build_pq first")
                if allowed_ids is not None or nprobe is not None or sq:
                    raise NotImplementedError("search(pq=True) takes no allowed_ids, no nprobe and no sq")
                dist, rows = self.pq.search(q.reshape(1, -1), k)
            elif sq:
                if self.sq is None:
                    raise RuntimeError("search(sq=True) needs build_sq first")
                if allowed_ids is not None or nprobe is not None:
                    raise NotImplementedError("search(sq=True) takes no allowed_ids and no nprobe")
                dist, rows = self.sq.search(q.reshape(1, -1), k)
            elif nprobe is not None:
                if self.ivf is None:
                    raise RuntimeError("search(nprobe=...) needs build_ivf first")
                if allowed_ids is not None:
                    raise NotImplementedError("search(nprobe=...) takes no allowed_ids")
                dist, rows = self.ivf.search(q.reshape(1, -1), k, params=_fx.SearchParametersIVF(nprobe=int(nprobe)))
            elif allowed_ids is None:
                dist, rows = self.index.search(q.reshape(1, -1), k)
            else:
                dist, rows = self.index.search(q.reshape(1, -1), k, params=self._rows_selector(allowed_ids))
            if not isinstance(dist, np.ndarray):  # device tensors -> host
                dist, rows = dist.cpu().numpy(), rows.cpu().numpy()
            n_ids = len(self.doc_ids)
            keep = [(float(dv), int(r)) for dv, r in zip(dist[0], rows[0]) if r != -1 and r < n_ids]
            found = [self.doc_ids[r] for _, r in keep]
            logger.info("search k=%d over %d rows -> %s", k, self.index.ntotal, found)
            return np.array([dv for dv, _ in keep], dtype=np.float32) if keep else np.array([]), found
        except Exception as e:  # noqa: BLE001 -- the reference swallows every error here
            logger.error("search failed: %s", e)
            return np.array([]), []

    def search_radius(self, query_vector, radius: float) -> Tuple[np.ndarray, List[int]]:
        """Every stored vector within squared L2 distance ``radius`` of one
        query (``index.range_search``; strict, exact membership) -- the
        thresholded form of ``search``: "every chunk with score >= s" is
        ``radius = 1/s - 1`` under the front ends' ``1 / (1 + d)``.  Rows map
        to document ids with ``search``'s filter (rows past the id list are
        dropped); results are sorted by (distance, row).  On any error the
        result is ``(np.array([]), [])``, as ``search``."""
        try:
            q = query_vector
            if isinstance(q, list):
                q = np.array(q, dtype=np.float32)
            _, dist, rows = self.index.range_search(q.reshape(1, -1), float(radius))
            if not isinstance(dist, np.ndarray):  # device tensors -> host
                dist, rows = dist.cpu().numpy(), rows.cpu().numpy()
            n_ids = len(self.doc_ids)
            keep = sorted((float(dv), int(r)) for dv, r in zip(dist, rows) if 0 <= r < n_ids)
            found = [self.doc_ids[r] for _, r in keep]
            logger.info("search_radius %g over %d rows -> %d hits", radius, self.index.ntotal, len(found))
            return np.array([dv for dv, _ in keep], dtype=np.float32) if keep else np.array([]), found
        except Exception as e:  # noqa: BLE001 -- same contract as search
            logger.error("search_radius failed: %s", e)
            return np.array([]), []

    def remove_vectors(self, ids) -> int:
        """Remove every row whose document id is in ``ids`` (extension; the
        index's ``remove_ids``: compacted in place on the GPU, the kept rows
        keep their order).  An id that occurs several times removes all its
        rows; unknown ids are ignored; rows past the end of ``doc_ids`` (see
        ``add_vectors``) are left alone.  The same positions go from
        ``doc_ids``, so rows and ids stay aligned.  Returns the number of rows
        removed.  Errors are logged and raised again, as in ``load_index``."""
        try:
            gone = set(int(a) for a in ids)
            n_rows = min(len(self.doc_ids), self.index.ntotal)
            rows = [r for r in range(n_rows) if self.doc_ids[r] in gone]
            if not rows:
                return 0
            self.ivf = self.sq = self.pq = None
            n = int(self.index.remove_ids(np.asarray(rows, dtype=np.int64)))
            dropped = set(rows)
            self.doc_ids = [doc for r, doc in enumerate(self.doc_ids) if r not in dropped]
            logger.info("remove: %d rows -> ntotal %d", n, self.index.ntotal)
            return n
        except Exception as e:
            logger.error("remove failed: %s", e)
            raise

    def cluster(self, k: int, niter: int = 25, seed: int = 1234) -> Tuple[np.ndarray, np.ndarray]:
        """Cluster the stored rows into ``k`` groups (extension; ``Kmeans`` of
        the faiss surface trained on the index itself, so the rows never leave
        the GPU).  Returns ``(centroids, labels)``: ``(k, d)`` fp32, and the
        cluster of every stored row as numpy int64, in row order.  Errors are
        logged and raised again, as in ``load_index``."""
        try:
            km = _fx.Kmeans(self.dimension, int(k), niter=int(niter), seed=int(seed), device=self.device)
            km.train(self.index)
            _, labels = km.assign(self.index)
            logger.info("cluster: %d rows -> %d clusters, objective %g", self.index.ntotal, k,
                        km.obj[-1] if len(km.obj) else 0.0)
            return km.centroids, labels
        except Exception as e:
            logger.error("cluster failed: %s", e)
            raise

    def save_index(self, filepath: Optional[str] = None):
        """faiss_store.py:83-97: IxF2 index file + pickle-protocol-4 id list
        at ``<path>.mapping``."""
        path = filepath or self.index_path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        _fx.write_index(self.index, path)
        with open(path + ".mapping", "wb") as f:
            f.write(_mapping.dumps_ids(self.doc_ids))
        logger.info("saved %d rows to %s", self.index.ntotal, path)

    def load_index(self, filepath: Optional[str] = None):
        """faiss_store.py:99-122: without a mapping file the ids are the row
        numbers; errors are logged and raised again."""
        path = filepath or self.index_path
        try:
            self.ivf = self.sq = self.pq = None
            self.index = _fx.read_index(path, dtype=self.dtype, device=self.device)
            if os.path.exists(path + ".mapping"):
                with open(path + ".mapping", "rb") as f:
                    self.doc_ids = _mapping.loads_ids(f.read())
            else:
                self.doc_ids = list(range(self.index.ntotal))
                logger.warning("%s.mapping missing: ids are the row numbers", path)
            logger.info("loaded %d rows, %d ids from %s", self.index.ntotal, len(self.doc_ids), path)
        except Exception as e:
            logger.error("load of %s failed: %s", path, e)
            raise

    def reset(self):
        """faiss_store.py:124-128: a fresh empty index, no ids."""
        self.ivf = self.sq = self.pq = None
        self.index = _fx.IndexFlatL2(self.dimension, dtype=self.dtype, device=self.device)
        self.doc_ids = []
        logger.info("reset")
