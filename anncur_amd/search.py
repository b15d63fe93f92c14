"""Search with a CUR index and a cross-encoder, without the exact [Q x I] score matrix.

The point of CUR retrieval is never to score all items with the cross-encoder.  A search is four steps:
  1. score the queries against the kc anchor items             -> X [Q x kc]      (kc scorer cells per query)
  2. retrieve k_retvr candidates from the index, anchors excluded (CURRowIndex.topk, exclude=)
  3. score those candidates with the cross-encoder             -> [Q x k_retvr]   (k_retvr scorer cells per query)
  4. the best k by exact score among anchors + candidates      (ops.rerank_scored)
The anchors' scores are paid for in step 1 and belong in the final pool (the reference's grids, ..._w_fixed_train_test_splits.py:238-251,
are laid out for comparisons at an equal budget of n_anc + k_retvr cross-encoder calls).

Scorer protocol -- any callable:

    scorer(query_ids, item_ids) -> scores on the device
        query_ids : int64 [Q]
        item_ids  : int32 [n]      one list for all queries  -> scores [Q x n]
                 or int32 [Q x n]  per query, -1 = hole      -> scores [Q x n]  (holes: any value)

MatrixScorer answers from a stored matrix: the evaluation stand-in for a model.
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .cur import _is_full_range

SearchResult = namedtuple("SearchResult", ["values", "indices", "n_scored"])


class MatrixScorer(object):
	"""The scorer protocol on a resident exact matrix A [n_queries x n_items] (fp32 or bf16, on the GPU): shared item lists through
	ops.gather_cols, per-query lists through ops.gather_pairs (a hole reads as NaN), both on the gathered query rows -- the full range
	0..n-1 takes A as it is."""

	def __init__(self, A_dev):
		self.A = A_dev

	def __call__(self, query_ids, item_ids):
		rows = self.A if _is_full_range(query_ids, self.A.shape[0]) else ops.gather_rows(self.A, query_ids)
		if item_ids.dim() == 1:
			return ops.gather_cols(rows, item_ids)
		return ops.gather_pairs(rows, item_ids)


class CrossEncoderSearcher(object):
	"""search(): the four steps above over a CURRowIndex and a scorer.

	anchors_in_pool=True (default): the retrieval excludes the anchor items (so all k_retvr candidates are NEW items), and the final pool
	is anchors + candidates; the scorer is never asked for an anchor twice, and n_scored = kc + k_retvr.  The index' anchor ids must be
	strictly ascending (ops.shared_id_list; the harness' anchor selection is): they are checked, and the exclusion normalised, once here.
	anchors_in_pool=False: the plain retrieval and a re-rank of its candidates alone -- ops.rerank without the matrix, today's evaluation
	cell, whose budget counts n_scored = k_retvr."""

	def __init__(self, index, scorer, anchors_in_pool=True):
		self.index, self.scorer, self.anchors_in_pool = index, scorer, bool(anchors_in_pool)
		dev = index.R.device
		anc = np.asarray(index.col_idxs.detach().cpu().numpy() if torch.is_tensor(index.col_idxs) else index.col_idxs, dtype=np.int64).reshape(-1)
		self.kc = int(anc.size)
		self._anchor_ids = ops.as_index(anc, dev, index.m)
		self._shared = self._excl = None
		if self.anchors_in_pool:
			self._shared = ops.shared_id_list(anc, dev)
			self._excl = ops.exclusion(anc, 0, index.m, dev)

	def search(self, query_ids, k, k_retvr):
		"""-> SearchResult(values f32 [Q x k], indices int32 [Q x k], n_scored): the k best by exact score, descending, ties by the
		smaller id, (-inf, -1) where the pool holds fewer than k scored items.  ValueError: k beyond min(pool size, ANNCUR_MAX_TOPK);
		in pool mode k_retvr + kc beyond what one filtered retrieval returns (ops.filtered_k)."""
		pool = k_retvr + (self.kc if self.anchors_in_pool else 0)
		limit = min(pool, ops._lib.MAX_TOPK)
		if k_retvr < 1 or k < 1 or k > limit:
			raise ValueError(f"search: need k_retvr >= 1 and 1 <= k <= min(pool size, ANNCUR_MAX_TOPK) = min({pool}, {ops._lib.MAX_TOPK}) = {limit} (got k = {k}, k_retvr = {k_retvr})")
		if self.anchors_in_pool and self._excl.e_max:
			ops.filtered_k(k_retvr, self._excl.e_max, self.index.m)   # (before the first scorer call: the ValueError the retrieval would raise)
		X = self.scorer(query_ids, self._anchor_ids)
		cand = self.index.topk(X, k_retvr, exclude=self._excl) if self.anchors_in_pool else self.index.topk(X, k_retvr)
		scores = self.scorer(query_ids, cand.indices)
		if scores.dtype != torch.float32:
			scores = ops.convert(scores, torch.float32)
		if self.anchors_in_pool:
			res = ops.rerank_scored(k, cand, scores, self._shared, X)
			return SearchResult(res.values, res.indices, self.kc + k_retvr)
		res = ops.rerank_scored(k, cand, scores)
		return SearchResult(res.values, res.indices, k_retvr)
