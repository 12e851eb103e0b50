"""Retrieval callers over the MI355X index.

The reference runs its two retrieval callers one query at a time, each with a
device round trip and a CPU faiss scan:

* ``RAGDatabaseManager.search_similar_documents(query, k=5)``
  (rag_datastore_manager.py:211-238, Stack A): encode -> ``faiss_index.search``
  -> re-read the pickled row->doc-id mapping from disk on EVERY query (:221-223)
  -> ``doc_ids[idx]`` (no -1 filter: a missing slot silently maps to the last
  document, :228) -> ``Database.fetch_document`` one row at a time (:229) ->
  ``doc['distance'] = float(d)``.  Any error -> ``[]`` (:236-238).
* ``QueryEngine.search(query, top_k=5)`` (query.py:21-55, Stack B): encode ->
  ``FAISSVectorStore.search`` (already maps rows to doc ids and drops -1,
  faiss_store.py:70-74) -> ``Database.get_document_by_id(int(idx) + 1)``
  (query.py:40 -- an off-by-one on ids that are already document ids) ->
  ``doc['score'] = 1 / (1 + distance)`` (query.py:42).  Any error -> ``[]``.

Here both take a BATCH of queries: one encoder pass (device-resident, no
per-batch ``.cpu()``), one fused scan for all queries, one SQLite ``IN``
lookup for all hits.  Result dictionaries keep the reference's keys and
order.  Deliberate differences, in this counterpart only:

* ``search_similar_documents`` drops ``I = -1`` slots instead of mapping them
  to ``doc_ids[-1]`` ("fix -1 handling in the build's own
  counterpart only"), and reads the mapping once, not per query;
* ``query_engine_search`` reproduces the ``+1`` of query.py:40 by default
  (``id_shift=1``) so a switched caller returns the same rows; pass
  ``id_shift=0`` for the corrected join.
"""
from __future__ import annotations

import logging
import sqlite3
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

logger = logging.getLogger("rag_faiss_embedding_amd.retrieval")

# column sets of the two reference schemas
_COLS_A = ("id", "url", "title", "content", "created_at", "updated_at")  # rag_datastore_manager.py:33-42
_COLS_B = ("id", "url", "title", "content")                             # database.py:60-72 row -> dict


def similarity(distance: float) -> float:
    """The score both reference front ends show: 1 / (1 + d)
    (query.py:42, 2-cli-rag-search.py:48)."""
    return float(1.0 / (1.0 + distance))


class DocumentStore:
    """Read side of the reference's SQLite ``documents`` table
    (rag_datastore_manager.py:22-97 / database.py:10-104), batched: one
    ``SELECT ... WHERE id IN (...)`` per search batch instead of one query
    per hit."""

    def __init__(self, conn_or_path, columns: Sequence[str] = _COLS_A):
        self.conn = conn_or_path if isinstance(conn_or_path, sqlite3.Connection) else sqlite3.connect(conn_or_path)
        self.columns = tuple(columns)

    def fetch_many(self, ids: Iterable[int]) -> Dict[int, Dict]:
        ids = sorted({int(i) for i in ids})
        out: Dict[int, Dict] = {}
        cols = ", ".join(self.columns)
        for lo in range(0, len(ids), 900):  # SQLite's bound-parameter limit
            chunk = ids[lo:lo + 900]
            q = f"SELECT {cols} FROM documents WHERE id IN ({','.join('?' * len(chunk))})"
            for row in self.conn.execute(q, chunk):
                out[int(row[0])] = dict(zip(self.columns, row))
        return out

    def count(self) -> int:
        return int(self.conn.execute("SELECT COUNT(*) FROM documents").fetchone()[0])


def _to_numpy(x) -> np.ndarray:
    if hasattr(x, "detach"):  # torch tensor (device results of a device search)
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def selector_for_documents(doc_ids: Sequence[int], allowed_ids: Iterable[int]):
    """``faiss.SearchParameters`` selecting the index rows whose document id is
    in ``allowed_ids`` (``doc_ids`` is the row -> document id mapping; an id
    held by several rows selects them all, an unknown id none)."""
    from . import faiss as fx
    allowed = np.fromiter((int(a) for a in allowed_ids), dtype=np.int64)
    rows = np.flatnonzero(np.isin(np.asarray(doc_ids, dtype=np.int64), allowed))
    return fx.SearchParameters(sel=fx.IDSelectorBatch(rows.astype(np.int64)))


def mmr_pick(sim_q: np.ndarray, vectors: np.ndarray, k: int, lam: float, l2: bool) -> List[int]:
    """Greedy maximal-marginal-relevance pick of ``k`` of n ranked candidates:
    repeatedly the candidate c with the largest

        lam * s(q, c) - (1 - lam) * max over picked p of s(c, p)

    where ``sim_q[c]`` = s(q, c) and s between candidates is ``-|c - p|^2``
    (``l2``) or the dot product, from ``vectors`` (n, d) in float64.  The first
    pick is rank 0; ties go to the earlier rank.  Returns the picked ranks in
    pick order."""
    n = len(sim_q)
    if n == 0 or k <= 0:
        return []
    sim_q = np.asarray(sim_q, dtype=np.float64)
    v = np.asarray(vectors, dtype=np.float64)

    def sim_to(p: int) -> np.ndarray:
        return -((v - v[p]) ** 2).sum(axis=1) if l2 else v @ v[p]

    picked = [0]
    closest = sim_to(0)  # every candidate's largest similarity to a picked one
    while len(picked) < min(int(k), n):
        value = lam * sim_q - (1.0 - lam) * closest
        value[picked] = -np.inf
        j = int(np.argmax(value))  # (the first maximum: the earlier rank)
        picked.append(j)
        closest = np.maximum(closest, sim_to(j))
    return picked


def _diverse_search(index, query_embeddings, k: int, params, diversity: float, fetch_k: Optional[int]):
    """``search`` re-ranked for diversity: ``fetch_k`` candidates (default 4k)
    and their stored vectors from one ``search_and_reconstruct``, then
    ``mmr_pick`` per query.  Returns (D, I) shaped (nq, k), missing slots -1."""
    lam = float(diversity)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"diversity must be in [0, 1] (got {diversity})")
    fetch = max(int(k), int(fetch_k) if fetch_k is not None else 4 * int(k))
    Dc, Ic, Rc = index.search_and_reconstruct(query_embeddings, fetch, params=params)
    Dc, Ic, Rc = _to_numpy(Dc), _to_numpy(Ic), _to_numpy(Rc)
    l2 = getattr(index, "metric_type", 1) == 1
    D = np.full((Ic.shape[0], int(k)), np.finfo(np.float32).max if l2 else -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((Ic.shape[0], int(k)), -1, dtype=np.int64)
    for qi in range(Ic.shape[0]):
        live = np.flatnonzero(Ic[qi] >= 0)  # (ranked first: missing slots pad the end)
        sim_q = -Dc[qi, live].astype(np.float64) if l2 else Dc[qi, live].astype(np.float64)
        picks = live[mmr_pick(sim_q, Rc[qi, live], int(k), lam, l2)]
        D[qi, :len(picks)] = Dc[qi, picks]
        I[qi, :len(picks)] = Ic[qi, picks]
    return D, I


def search_similar_documents(index, doc_ids: Sequence[int], store: DocumentStore, query_embeddings,
                             k: int = 5, allowed_ids: Optional[Iterable[int]] = None,
                             diversity: Optional[float] = None, fetch_k: Optional[int] = None) -> List[List[Dict]]:
    """Batched ``RAGDatabaseManager.search_similar_documents``
    (rag_datastore_manager.py:211-238): for every query row, the documents
    of its k nearest index rows, nearest first, each with ``distance`` (the
    squared L2 distance the index returned).  ``doc_ids`` is the row -> doc
    id mapping (faiss_index.bin.mapping).  ``allowed_ids`` (document ids):
    only those documents are ranked, by the index's filtered search.
    ``diversity`` (lambda in [0, 1]; None: off): the k results are picked
    greedily by maximal marginal relevance (``mmr_pick``) among the
    ``fetch_k`` (default 4k) nearest rows, whose vectors come from the
    index's ``search_and_reconstruct``; 1 is the plain ranking, smaller
    values trade nearness for spread.  Errors are logged and give empty
    lists, as the reference's blanket ``except`` does."""
    try:
        params = None if allowed_ids is None else selector_for_documents(doc_ids, allowed_ids)
        if diversity is not None:
            D, I = _diverse_search(index, query_embeddings, int(k), params, diversity, fetch_k)
        elif allowed_ids is None:
            D, I = index.search(query_embeddings, int(k))
        else:
            D, I = index.search(query_embeddings, int(k), params=params)
        D, I = _to_numpy(D), _to_numpy(I)
        ids = np.asarray(doc_ids, dtype=np.int64)
        valid = (I >= 0) & (I < len(ids))
        docs = store.fetch_many(ids[I[valid]].tolist())
        results: List[List[Dict]] = []
        for qi in range(I.shape[0]):
            row: List[Dict] = []
            for idx, dist in zip(I[qi], D[qi]):
                if idx < 0 or idx >= len(ids):
                    continue  # faiss pads missing slots with -1 (see module note)
                doc = docs.get(int(ids[idx]))
                if doc is not None:
                    d = dict(doc)
                    d["distance"] = float(dist)
                    row.append(d)
            results.append(row)
        return results
    except Exception as e:  # noqa: BLE001 -- reference contract (rag_datastore_manager.py:236-238)
        logger.error("Error searching documents: %s", e)
        n = getattr(query_embeddings, "shape", [1])[0] if hasattr(query_embeddings, "shape") else 1
        return [[] for _ in range(n)]


def query_engine_search(store_index, store: DocumentStore, query_embeddings, top_k: int = 5,
                        id_shift: int = 1) -> List[List[Dict]]:
    """Batched ``QueryEngine.search`` (query.py:21-55) over a
    ``FAISSVectorStore``-like object (``.index`` + ``.doc_ids``): vector
    search, the join ``get_document_by_id(doc_id + id_shift)`` (query.py:40
    uses +1) and ``score = 1 / (1 + distance)``.  Returns one list per query;
    errors give empty lists (query.py:53-55)."""
    try:
        D, I = store_index.index.search(query_embeddings, int(top_k))
        D, I = _to_numpy(D), _to_numpy(I)
        ids = np.asarray(store_index.doc_ids, dtype=np.int64)
        valid = (I >= 0) & (I < len(ids))          # faiss_store.py:70-73
        docs = store.fetch_many((ids[I[valid]] + id_shift).tolist())
        results: List[List[Dict]] = []
        for qi in range(I.shape[0]):
            row: List[Dict] = []
            for idx, dist in zip(I[qi], D[qi]):
                if idx < 0 or idx >= len(ids):
                    continue
                doc = docs.get(int(ids[idx]) + id_shift)
                if doc is not None:
                    d = dict(doc)
                    d["score"] = similarity(float(dist))
                    row.append(d)
            results.append(row)
        return results
    except Exception as e:  # noqa: BLE001 -- reference contract
        logger.exception("Search error: %s", e)
        n = query_embeddings.shape[0] if hasattr(query_embeddings, "shape") else 1
        return [[] for _ in range(n)]


def radius_for_score(min_score: float) -> float:
    """The L2 radius of ``score >= min_score`` under ``similarity``:
    1 / (1 + d) >= s  <=>  d <= 1/s - 1, for 0 < s <= 1."""
    s = float(min_score)
    if not 0.0 < s <= 1.0:
        raise ValueError(f"min_score must be in (0, 1] (got {min_score})")
    return 1.0 / s - 1.0


def documents_within(index, doc_ids: Sequence[int], store: DocumentStore, query_embeddings, *,
                     max_distance: Optional[float] = None, min_score: Optional[float] = None) -> List[List[Dict]]:
    """Every document within a threshold of each query row, nearest first
    (ties: smaller index row) -- "every chunk with score >= 0.6" instead of
    "the best 5, however bad".  Exactly one of ``max_distance`` (the index's
    radius: squared L2 distance, strict) and ``min_score`` (the front ends'
    ``1 / (1 + d)``, L2 indexes only; radius ``1/s - 1``) is given.  One
    ``index.range_search`` and one ``fetch_many`` per batch; each document
    carries ``distance`` and ``score``.  Errors are logged and give empty
    lists, as the other callers here."""
    try:
        if (max_distance is None) == (min_score is None):
            raise ValueError("give exactly one of max_distance and min_score")
        if min_score is not None:
            if getattr(index, "metric_type", 1) != 1:
                raise ValueError("min_score needs an L2 index")
            radius = radius_for_score(min_score)
        else:
            radius = float(max_distance)
        lims, D, I = index.range_search(query_embeddings, radius)
        lims, D, I = _to_numpy(lims).astype(np.int64), _to_numpy(D), _to_numpy(I)
        ids = np.asarray(doc_ids, dtype=np.int64)
        valid = (I >= 0) & (I < len(ids))
        docs = store.fetch_many(ids[I[valid]].tolist())
        results: List[List[Dict]] = []
        for qi in range(len(lims) - 1):
            lo, hi = int(lims[qi]), int(lims[qi + 1])
            row: List[Dict] = []
            for dist, idx in sorted(zip(D[lo:hi].tolist(), I[lo:hi].tolist())):
                if idx < 0 or idx >= len(ids):
                    continue
                doc = docs.get(int(ids[idx]))
                if doc is not None:
                    d = dict(doc)
                    d["distance"] = float(dist)
                    d["score"] = similarity(float(dist))
                    row.append(d)
            results.append(row)
        return results
    except Exception as e:  # noqa: BLE001 -- same contract as search_similar_documents
        logger.error("Error searching documents within a radius: %s", e)
        n = getattr(query_embeddings, "shape", [1])[0] if hasattr(query_embeddings, "shape") else 1
        return [[] for _ in range(n)]


class RetrievalEngine:
    """Encoder + index + document store: the retrieval half of the
    reference's CLI / QueryEngine, batched.  ``search(texts, k)`` encodes all
    texts in one device-resident pass and scans the index once."""

    def __init__(self, vectorizer, index, doc_ids: Sequence[int], store: DocumentStore):
        self.vectorizer = vectorizer
        self.index = index
        self.doc_ids = list(doc_ids)
        self.store = store

    def embed(self, texts: List[str]):
        if hasattr(self.vectorizer, "generate_embeddings_device"):
            return self.vectorizer.generate_embeddings_device(texts)
        return np.asarray(self.vectorizer.generate_embeddings(texts), dtype=np.float32)

    def search(self, texts: List[str], k: int = 5, allowed_ids: Optional[Iterable[int]] = None,
               diversity: Optional[float] = None, fetch_k: Optional[int] = None) -> List[List[Dict]]:
        """``allowed_ids``: rank only these document ids (filtered search).
        ``diversity`` / ``fetch_k``: maximal-marginal-relevance re-ranking
        (``search_similar_documents``)."""
        if not texts:
            return []
        if diversity is None:
            return search_similar_documents(self.index, self.doc_ids, self.store, self.embed(texts), k,
                                            allowed_ids=allowed_ids)
        return search_similar_documents(self.index, self.doc_ids, self.store, self.embed(texts), k,
                                        allowed_ids=allowed_ids, diversity=diversity, fetch_k=fetch_k)

    def search_within(self, texts: List[str], *, max_distance: Optional[float] = None,
                      min_score: Optional[float] = None) -> List[List[Dict]]:
        """Every document within ``max_distance`` (or scoring at least
        ``min_score``) of each text: ``documents_within`` over one encoder pass."""
        if not texts:
            return []
        return documents_within(self.index, self.doc_ids, self.store, self.embed(texts),
                                max_distance=max_distance, min_score=min_score)

    def remove_documents(self, ids: Iterable[int]) -> int:
        """Remove every index row whose document id is in ``ids`` (all rows of
        an id held by several; unknown ids are ignored; rows past the end of
        ``doc_ids`` are left alone) and the same positions of the engine's own
        ``doc_ids`` list.  Returns the number of rows removed.  Errors
        propagate."""
        gone = np.fromiter((int(a) for a in ids), dtype=np.int64)
        n_rows = min(len(self.doc_ids), int(self.index.ntotal))
        rows = np.flatnonzero(np.isin(np.asarray(self.doc_ids[:n_rows], dtype=np.int64), gone)).astype(np.int64)
        if rows.size == 0:
            return 0
        n = int(self.index.remove_ids(rows))
        dropped = set(rows.tolist())
        self.doc_ids = [doc for r, doc in enumerate(self.doc_ids) if r not in dropped]
        return n

    def search_one(self, text: str, k: int = 5) -> List[Dict]:
        """The reference's single-query call shape (rag_datastore_manager.py:211)."""
        out = self.search([text], k)
        return out[0] if out else []


def load_store_and_mapping(db_path: str, mapping_path: str, columns: Optional[Sequence[str]] = None):
    """(DocumentStore, doc_ids) from the reference's on-disk artefacts:
    ``data/documents.db`` and ``data/faiss_index.bin.mapping`` (parsed
    without unpickling, see _mapping.py)."""
    from pathlib import Path

    from ._mapping import loads_ids
    return DocumentStore(db_path, columns or _COLS_A), loads_ids(Path(mapping_path).read_bytes())
