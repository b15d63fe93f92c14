"""Device-side replacement of the reference's per-query evaluation loop
(eval/run_retrieval_eval_wrt_exact_crossenc.py:97-154 and
 eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py:51-206):
exact top-k scan, approximate top-k_retvr, exact re-rank, overlap statistics.
One exact scan and one retrieval at the largest k serve every (top_k, k_retvr) cell of a sweep."""
import numpy as np
import torch

from . import ops
from .eval_utils import flatten_overlap, overlap_stats_batch, overlap_stats_from_counts


def exact_topk(A_dev, k):
	return ops.rowwise_topk(A_dev, k)


def overlap_cells(exact_idx, approx_idx, cells, A_dev=None, literal_rerank=False):
	"""common counts [n_cells, Q] for cells = [(top_k, k_retvr), ...].

	Closed form (default): |exact[:top_k] & rerank_{k_retvr}[:top_k]| == |exact[:top_k] & approx[:k_retvr]|
	because both rankings break ties the same way (score desc, index asc).  literal_rerank=True runs the
	re-rank kernel per k_retvr exactly like the reference's scatter + topk (tests check both agree)."""
	if not literal_rerank:
		return ops.overlap_counts(exact_idx, approx_idx, cells)
	out = torch.empty((len(cells), exact_idx.shape[0]), dtype=torch.int32, device=exact_idx.device)
	for kr in sorted({c[1] for c in cells}):
		sel = [j for j, c in enumerate(cells) if c[1] == kr]
		kmax = max(cells[j][0] for j in sel)
		rr = ops.rerank(A_dev, approx_idx, kr, kmax)
		cnt = ops.overlap_counts(exact_idx, rr.indices, [(cells[j][0], cells[j][0]) for j in sel])
		for r, j in enumerate(sel):
			out[j] = cnt[r]
	return out


# ------------------------------------------------------------------ the recall curve from ranks
def _host_ranks(ranks):
	r = ranks.detach().cpu().numpy() if torch.is_tensor(ranks) else np.asarray(ranks)
	if r.ndim != 2 or r.dtype.kind not in "iu":
		raise ValueError("ranks must be an integer [Q x k] array (index.rank_of(X, exact.indices[:, :k]))")
	return r


def overlap_from_ranks(ranks, cells):
	"""common counts [n_cells, Q] (NumPy int32) for cells = [(top_k, k_retvr), ...] from ranks [Q x >= max top_k], the approximate rank of each
	query's exact top-k items in exact order (index.rank_of(X, exact.indices)): #{j < top_k : 0 <= ranks[q, j] < k_retvr} -- what overlap_cells
	counts from a retrieved list, for ANY k_retvr up to n_ent and without that list.  A rank of -1 (a hole, a NaN score) is never retrieved."""
	r = _host_ranks(ranks)
	out = np.empty((len(cells), r.shape[0]), dtype=np.int32)
	for j, (k, kr) in enumerate(cells):
		if not 0 <= k <= r.shape[1]:
			raise ValueError(f"overlap_from_ranks: cell ({k}, {kr}) needs {k} ranks per query, {r.shape[1]} given")
		out[j] = ((r[:, :k] >= 0) & (r[:, :k] < kr)).sum(axis=1)
	return out


RANK_CURVE_RECALLS = (0.5, 0.9, 0.95, 0.99, 1.0)
RANK_CURVE_PREFIX = "exact_topk_approx_rank"


def _nth_smallest(sorted_vals, frac, n):
	"""The ceil(frac n)-th smallest of the n pairs (the product taken exactly, not in binary floating point), None where it falls among
	the pairs without a rank (sorted_vals holds only the ranked ones)."""
	from fractions import Fraction
	m = max(1, -((-Fraction(str(frac)) * n) // 1))
	return int(sorted_vals[m - 1]) if m <= len(sorted_vals) else None


def rank_curve(ranks, top_k_vals, recalls=RANK_CURVE_RECALLS):
	"""{top_k: metrics} from ranks [Q x >= max top_k] (as for overlap_from_ranks), over all Q top_k pairs (query, exact top-k item):
	  exact_topk_approx_rank~mean                 mean rank (0-based) of the ranked pairs, rounded to 4 decimals
	  exact_topk_approx_rank~p50 / p90 / p99      the ceil(p Q k)-th smallest rank (nearest-rank percentile, an integer)
	  exact_topk_approx_rank~max                  the largest rank
	  k_retvr_for_recall~{r}                      the ceil(r Q k)-th smallest rank, plus 1: the smallest k_retvr whose retrieved lists hold
	                                              that fraction of all exact top-k items
	A pair without a rank (-1) counts as never retrieved: it is left out of mean and max, and a percentile or recall level that falls among
	such pairs is None."""
	r = _host_ranks(ranks)
	out = {}
	for k in top_k_vals:
		if not 1 <= k <= r.shape[1]:
			raise ValueError(f"rank_curve: top_k = {k} needs {k} ranks per query, {r.shape[1]} given")
		flat = r[:, :k].reshape(-1)
		n = flat.size
		s = np.sort(flat[flat >= 0].astype(np.int64))
		m = {f"{RANK_CURVE_PREFIX}~mean": round(float(s.mean()), 4) if s.size else None}
		for name, frac in (("p50", 0.5), ("p90", 0.9), ("p99", 0.99)):
			m[f"{RANK_CURVE_PREFIX}~{name}"] = _nth_smallest(s, frac, n) if n else None
		m[f"{RANK_CURVE_PREFIX}~max"] = int(s[-1]) if s.size else None
		for frac in recalls:
			v = _nth_smallest(s, frac, n) if n else None
			m[f"k_retvr_for_recall~{frac}"] = None if v is None else v + 1
		out[k] = m
	return out


# ------------------------------------------------------------------ the pool "retrieved + anchors" 
POOL_PREFIX = "exact_vs_reranked_approx_retvr_w_anchors"
OVERLAP_MAX_LIST = 4096   # longest list anncur_overlap_counts takes


def pool_cell_limit(n_ent):
	"""Largest n_anc + k_retvr of a pool cell: the retrieval with the anchors excluded asks one top-k call for k_retvr + n_anc candidates
	(ops.filtered_k: at most min(n_ent, ANNCUR_MAX_TOPK)), and the pool is one list of the overlap kernel (at most 4096 ids)."""
	return min(n_ent, ops._lib.MAX_TOPK, OVERLAP_MAX_LIST)


def split_pool_cells(cells, n_anc, n_ent):
	"""cells = [(top_k, k_retvr), ...] -> (cells the pool mode reports, cells it leaves out): k_retvr counts NEW items, so a cell needs
	k_retvr + n_anc <= pool_cell_limit(n_ent)."""
	limit = pool_cell_limit(n_ent)
	kept = [c for c in cells if c[1] + n_anc <= limit]
	return kept, [c for c in cells if c[1] + n_anc > limit]


def pool_pairs(cells, n_anc):
	"""Prefix-length pairs of the closed form over the list of pool_list: (top_k, n_anc + k_retvr) per cell."""
	return [(k, n_anc + kr) for k, kr in cells]


def pool_list(anchor_ids, retrieved_idx):
	"""[Q x (n_anc + k_retvr_max)] int32: the anchor ids FIRST (the same in every row), then the retrieved ids in retrieval order -- the
	pool of a cell (top_k, k_retvr) is the prefix of length n_anc + k_retvr."""
	Q = retrieved_idx.shape[0]
	anc = torch.as_tensor(anchor_ids, dtype=torch.int32, device=retrieved_idx.device).reshape(1, -1)
	return torch.cat([anc.expand(Q, anc.shape[1]), retrieved_idx.to(torch.int32)], dim=1).contiguous()


def overlap_pool_cells(exact_idx, anchor_ids, retrieved_idx, cells, A_dev=None, literal_rerank=False):
	"""common counts [n_cells, Q] of the pool mode for cells = [(top_k, k_retvr), ...]: the pool of a query is the anchor items plus its
	first k_retvr retrieved items (retrieved_idx: a retrieval with the anchors EXCLUDED, so they are new items).

	Closed form (default): |exact[:top_k] & rerank(pool)[:top_k]| == |exact[:top_k] & pool| (the argument of overlap_cells), one
	ops.overlap_counts call on pool_list / pool_pairs.  literal_rerank=True scores the pool like a search does -- anchors as one shared
	list, candidates per query, from MatrixScorer(A_dev) -- and runs ops.rerank_scored per k_retvr (tests check both agree)."""
	anchor_ids = np.asarray(anchor_ids, dtype=np.int64).reshape(-1)
	if not literal_rerank:
		return ops.overlap_counts(exact_idx, pool_list(anchor_ids, retrieved_idx), pool_pairs(cells, anchor_ids.size))
	from .search import MatrixScorer
	scorer = MatrixScorer(A_dev)
	qids = np.arange(A_dev.shape[0], dtype=np.int64)
	retrieved_idx = retrieved_idx.to(torch.int32).contiguous()
	shared = ops.shared_id_list(anchor_ids, A_dev.device) if anchor_ids.size else None
	X = scorer(qids, shared.ids) if shared is not None else None
	scores = scorer(qids, retrieved_idx)
	if scores.dtype != torch.float32:
		scores = ops.convert(scores, torch.float32)
	out = torch.empty((len(cells), exact_idx.shape[0]), dtype=torch.int32, device=exact_idx.device)
	for kr in sorted({c[1] for c in cells}):
		sel = [j for j, c in enumerate(cells) if c[1] == kr]
		kmax = max(cells[j][0] for j in sel)
		rr = ops.rerank_scored(kmax, retrieved_idx[:, :kr], scores[:, :kr], shared, X)
		cnt = ops.overlap_counts(exact_idx, rr.indices, [(cells[j][0], cells[j][0]) for j in sel])
		for r, j in enumerate(sel):
			out[j] = cnt[r]
	return out


def eval_topk_recall(A_dev, approx_idx, top_k_vals, k_retvr_vals, exact=None, row_subsets=None, literal_rerank=False):
	"""-> {(top_k, k_retvr): {"exact_vs_reranked_approx_retvr~common_mean": ..., ...}} in the reference's
	metric names and 4-decimal rounding.  approx_idx [Q, >= max k_retvr] sorted by approximate score.
	row_subsets: optional {name: index array}; then the value is {name: metrics} (entry point A's
	anchor / non_anchor / all split)."""
	cells = [(k, kr) for kr in k_retvr_vals for k in top_k_vals if k <= kr]
	if not cells:
		return {}
	kmax = max(k for k, _ in cells)
	if exact is None:
		exact = exact_topk(A_dev, kmax)
	counts = overlap_cells(exact.indices, approx_idx, cells, A_dev, literal_rerank).cpu().numpy()
	res = {}
	for j, (k, kr) in enumerate(cells):
		if row_subsets is None:
			res[(k, kr)] = flatten_overlap(overlap_stats_from_counts(counts[j], k))
		else:
			res[(k, kr)] = {name: flatten_overlap(overlap_stats_from_counts(counts[j][np.asarray(rows, dtype=np.int64)], k))
							for name, rows in row_subsets.items()}
	return res
