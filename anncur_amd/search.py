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

AdaptiveSearcher spends the same budget in several rounds: steps 2 and 3 repeat, and from the second round on the weights of
the retrieval are re-fitted per query on everything that query has scored so far (ops.lstsq_rows).
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .cur import SAMPLE_ROUTE, _is_full_range

SearchResult = namedtuple("SearchResult", ["values", "indices", "n_scored"])
AdaptiveResult = namedtuple("AdaptiveResult", ["values", "indices", "n_scored", "n_fallback", "trace"])


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


def adaptive_limits(kc, kq, m, k, k_step, n_rounds, incremental=False):
	"""The host checks of AdaptiveSearcher.search, on plain integers (kc anchor items, kq anchor queries, m items): a ValueError that
	names the limit, or None.  The evaluation harness asks the same question per grid cell.  incremental: the checks of
	AdaptiveSearcher(incremental=True) on top -- its solver state has the item side only."""
	max_topk, max_g = ops._lib.MAX_TOPK, ops._lib.LSTSQ_MAX_G
	if n_rounds < 1 or k_step < 1:
		raise ValueError(f"adaptive search: need n_rounds >= 1 and k_step >= 1 (got n_rounds = {n_rounds}, k_step = {k_step})")
	pool = kc + n_rounds * k_step
	if pool > min(m, max_topk):
		raise ValueError(f"adaptive search: kc + n_rounds * k_step = {kc} + {n_rounds} * {k_step} = {pool} scored items per query, above the limit of "
						 f"min(items, ANNCUR_MAX_TOPK) = min({m}, {max_topk}) = {min(m, max_topk)} of the last round's filtered retrieval")
	g = min(kc + (n_rounds - 1) * k_step, kq)
	if n_rounds >= 2 and g > max_g:
		raise ValueError(f"adaptive search: min(kc + (n_rounds - 1) * k_step, kq) = min({kc + (n_rounds - 1) * k_step}, {kq}) = {g}, above "
						 f"ANNCUR_LSTSQ_MAX_G = {max_g} of the per-query solve")
	if n_rounds >= 2 and kq > ops._lib.LSTSQ_MAX_KQ:
		raise ValueError(f"adaptive search: kq = {kq} anchor queries, above ANNCUR_LSTSQ_MAX_KQ = {ops._lib.LSTSQ_MAX_KQ}")
	if incremental and n_rounds >= 2 and kc + (n_rounds - 1) * k_step > kq:
		raise ValueError(f"adaptive search: incremental=True keeps a per-query factorisation of kc + (n_rounds - 1) * k_step = {kc} + {n_rounds - 1} * {k_step} = "
						 f"{kc + (n_rounds - 1) * k_step} scored items, above kq = {kq} anchor queries: the query side of the solve has no incremental form "
						 f"(use incremental=False)")
	if k < 1 or k > min(pool, max_topk):
		raise ValueError(f"adaptive search: need 1 <= k <= min(pool size, ANNCUR_MAX_TOPK) = min({pool}, {max_topk}) = {min(pool, max_topk)} (got k = {k})")


STRATEGIES = ("topk", "softmax")   # how a round of the adaptive search picks its new items


class AdaptiveSearcher(object):
	"""The multi-round search of DESIGN 4.4d ("Adaptive Selection of Anchor Items for CUR-based k-NN search with Cross-Encoders"): the
	budget of kc + n_rounds * k_step scorer cells per query is spent in rounds, and the items scored in round r become additional anchor
	items of THAT query in round r + 1:

	    s_hat_q = c_q . pinv(R[:, S_q]) . R        R = the index' anchor-query rows [kq x m], S_q = the items scored so far, c_q their scores

	round 0   X = scorer(query_ids, anchors); S_q = the anchor items
	round 1   index.topk(X, k_step, exclude=anchors) -- CrossEncoderSearcher's call, so n_rounds = 1 IS CrossEncoderSearcher.search
	round r   W = ops.lstsq_rows(Rt, S_q, c_q, ridge); the k_step best of W . R outside S_q (the index' routes on Rt as item operand,
	          exclude = the id-sorted S_q); score them; append and ops.sort_id_rows
	end       ops.rerank_scored(k, every item scored in rounds 1..n, anchors with X)
	Queries whose solve reports status != 0 (rank-deficient R[:, S_q]) -- and only they -- get w_q from numpy.linalg.pinv in fp64 on the host,
	the policy of cur._pinv for ill-conditioned blocks; n_fallback is the number of such queries.  The scorer is never asked for a
	(query, item) pair twice.  One host look per round r >= 2: the solve's status flags.

	incremental=True (opt-in; needs kc + (n_rounds - 1) k_step <= kq): the rounds r >= 2 keep S_q and c_q in INSERTION order -- the anchors
	in the index' order, then every round's candidates in retrieval order -- and solve on one ops.LstsqState of capacity
	kc + (n_rounds - 1) k_step, which factors only the positions a round appends (kc + k_step in round 2, k_step afterwards).  W is,
	bit for bit, ops.lstsq_rows on the same ordered rows; against incremental=False the unknowns are permuted, so the weights agree to
	rounding only.  The id-sorted copy is kept for the exclusion alone.  A failed query stays failed in the state: it takes the host
	fallback in every later round and is counted once.
	seed_shared=True (the default; only read with incremental=True): every query's rows begin with the same kc anchor items, so the state is
	seeded with them (ops.LstsqState.seed_shared: their kc x kc block is factored once, not once per query) and round 2 extends it by
	k_step positions like every later round.  Bit-equal to seed_shared=False, which absorbs kc + k_step positions per query in round 2.

	strategy: how a round picks its k_step new items (the paper names both).  "topk" (default): the k_step best of s_hat_q outside S_q --
	everything above, bit for bit.  "softmax": k_step items drawn without replacement with probability proportional to
	softmax(s_hat_q / temperature) outside S_q -- EVERY round, the first included: index.sample on X . E in round 1, the operand's sample on
	W . R afterwards (Gumbel top-k on the fp32 item operand, one dense route whatever compute_dtype is).  The noise of round r
	is drawn from (seed, stream = r, row key = the low 32 bits of the query's id, item id): a search is reproducible, and a query draws the
	same items wherever it stands in query_ids.  n_rounds = 1 with "softmax" is a sampled single round, no longer
	CrossEncoderSearcher.search.  The exclusion, the limits (adaptive_limits; the sampler takes k_step directly, so no k + e retrieval and no
	ops.filtered_k), the solves and the final re-rank are the same; it works with and without incremental=True."""

	def __init__(self, index, scorer, ridge=0.0, incremental=False, strategy="topk", temperature=1.0, seed=0, seed_shared=True):
		if strategy not in STRATEGIES:
			raise ValueError(f"AdaptiveSearcher: strategy = {strategy!r}, need one of {STRATEGIES}")
		self.strategy, self.temperature = strategy, ops._temperature_arg(temperature, "AdaptiveSearcher")
		self.seed = ops._noise_args(seed, 0, "AdaptiveSearcher")[0]
		self.index, self.scorer, self.ridge, self.incremental = index, scorer, float(ridge), bool(incremental)
		self.seed_shared = bool(seed_shared)
		if not self.ridge >= 0.0:
			raise ValueError(f"AdaptiveSearcher: ridge = {ridge}, need ridge >= 0")
		dev = index.R.device
		anc = np.asarray(index.col_idxs.detach().cpu().numpy() if torch.is_tensor(index.col_idxs) else index.col_idxs, dtype=np.int64).reshape(-1)
		self.kc, self.kq = int(anc.size), int(index.R.shape[0])
		self._anchor_ids = ops.as_index(anc, dev, index.m)
		self._shared = ops.shared_id_list(anc, dev)
		self._excl = ops.exclusion(anc, 0, index.m, dev)

	def _fallback(self, Rt, ids, scores, W, status):
		"""w_q = c_q . pinv(R_S) (ridge: the regularised normal equations) in fp64 on the host for the rows with status != 0 -> their row
		numbers (the round's one host look: an empty tensor almost always)."""
		bad = torch.nonzero(status).view(-1)
		if bad.numel() == 0:
			return bad
		Rt_h = Rt.detach().cpu().numpy().astype(np.float64)
		ids_h, sc_h = ids[bad].cpu().numpy(), scores[bad].cpu().numpy().astype(np.float64)
		rows = np.empty((bad.numel(), Rt_h.shape[1]), dtype=np.float32)
		for r in range(bad.numel()):
			keep = ids_h[r] >= 0
			Rs = Rt_h[ids_h[r][keep]].T                                   # kq x n_q
			if self.ridge > 0.0:
				w = np.linalg.solve(Rs @ Rs.T + self.ridge * np.eye(Rs.shape[0]), Rs @ sc_h[r][keep])
			else:
				w = sc_h[r][keep] @ np.linalg.pinv(Rs)
			rows[r] = w.astype(np.float32)
		W[bad] = torch.from_numpy(rows).to(W.device)
		return bad

	def _candidates(self, op, X, k_step, excl, r, row_keys):
		"""Round r's k_step new items from `op` (the index in round 1, its adaptive operand afterwards) by the searcher's strategy."""
		if self.strategy == "softmax":
			return op.sample(X, k_step, self.temperature, self.seed, r, row_keys, excl)
		return op.topk(X, k_step, exclude=excl)

	def search(self, query_ids, k, k_step, n_rounds, trace=False):
		"""-> AdaptiveResult(values f32 [Q x k], indices int32 [Q x k], n_scored = kc + n_rounds * k_step, n_fallback, trace): the k best by
		exact score among the anchors and everything the rounds scored, descending, ties by the smaller id.  ValueError (adaptive_limits,
		before the first scorer call) names the limit.  trace=True: a list with one dict per round r >= 2 -- "ids", "scores" (the id-sorted
		S_q and its scores the round solved on), "W" (after the host fallback), "status", "candidates" (the TopK retrieved, or the sampler's
		perturbed keys and items), "route" ("sample-dense" for a sampled round) --
		all tensors on the device; with incremental=True also "order_ids" and "order_scores", the rows in insertion order that the solve
		was given ("ids" / "scores" then hold the same pairs sorted, as the exclusion takes them)."""
		adaptive_limits(self.kc, self.kq, self.index.m, k, k_step, n_rounds, self.incremental)
		soft = self.strategy == "softmax"
		row_keys = ops._row_keys(query_ids, len(query_ids), self._anchor_ids.device, "adaptive search") if soft else None
		X = self.scorer(query_ids, self._anchor_ids)
		cand = self._candidates(self.index, X, k_step, self._excl, 1, row_keys)
		scores = self.scorer(query_ids, cand.indices)
		if scores.dtype != torch.float32:
			scores = ops.convert(scores, torch.float32)
		n_scored, log = self.kc + n_rounds * k_step, ([] if trace else None)
		if n_rounds == 1:
			res = ops.rerank_scored(k, cand, scores, self._shared, X)
			return AdaptiveResult(res.values, res.indices, n_scored, 0, log)
		Q = X.shape[0]
		fell_back = set()                                                   # queries solved on the host in any round
		operand = self.index.adaptive_operand()
		Rt = operand._Et
		Xf = X if X.dtype == torch.float32 else ops.convert(X, torch.float32)
		new_ids, new_scores = cand.indices, scores                        # every item scored in rounds 1.., in retrieval order
		S_ids = torch.cat([self._anchor_ids.view(1, -1).expand(Q, -1), new_ids], dim=1)
		state = O_ids = O_sc = None
		if self.incremental:
			O_ids, O_sc = S_ids.contiguous(), torch.cat([Xf, scores], dim=1)   # insertion order: what the state absorbs
			state = ops.LstsqState(Rt, Q, self.kc + (n_rounds - 1) * k_step, self.ridge)
			if self.seed_shared:
				state.seed_shared(self._anchor_ids)                           # the anchors' block: factored once for all queries
		S_ids, S_sc, counts = ops.sort_id_rows(S_ids, torch.cat([Xf, scores], dim=1))
		for r in range(2, n_rounds + 1):
			if state is None:
				W, status = ops.lstsq_rows(Rt, S_ids, S_sc, self.ridge)
			else:
				W, status = state.extend(O_ids, O_sc)
			fell_back.update(self._fallback(Rt, S_ids, S_sc, W, status).tolist())
			excl = ops.exclusion_from_sorted_rows(S_ids, counts)
			cand = self._candidates(operand, W, k_step, excl, r, row_keys)
			scores = self.scorer(query_ids, cand.indices)
			if scores.dtype != torch.float32:
				scores = ops.convert(scores, torch.float32)
			if trace:
				log.append({"ids": S_ids, "scores": S_sc, "W": W, "status": status, "candidates": cand, "route": SAMPLE_ROUTE if soft else operand.route(Q, k_step, excl)})
				if state is not None:
					log[-1].update({"order_ids": O_ids, "order_scores": O_sc})
			new_ids, new_scores = torch.cat([new_ids, cand.indices], dim=1), torch.cat([new_scores, scores], dim=1)
			if state is not None and r < n_rounds:
				O_ids, O_sc = torch.cat([O_ids, cand.indices], dim=1), torch.cat([O_sc, scores], dim=1)
			if r < n_rounds or trace:
				S_ids, S_sc, counts = ops.sort_id_rows(torch.cat([S_ids, cand.indices], dim=1), torch.cat([S_sc, scores], dim=1))
		if trace:
			log.append({"ids": S_ids, "scores": S_sc})                      # the final S_q
		res = ops.rerank_scored(k, new_ids, new_scores, self._shared, X)
		return AdaptiveResult(res.values, res.indices, n_scored, len(fell_back), log)
