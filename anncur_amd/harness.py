"""Evaluation harness of the two reference entry points, on the GPU.

Entry point A  (eval/run_retrieval_eval_wrt_exact_crossenc.py:47-200): anchors from ONE matrix, methods cur / cur_oracle,
                metrics split into anchor / non_anchor / all query rows, mean over seeds.
Entry point B  (eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py:209-443): index from the TRAIN
                matrix, test queries contribute their anchor-item scores, full (k_retvr x n_anchor) sweep.
The per-query Python loop of the reference (3 x topk + scatter per query) is replaced by one exact scan, one fused retrieval
at the largest k_retvr and one overlap kernel per sweep; results keep the reference's names, nesting and 4-decimal rounding.
"""
import itertools
import logging
import pickle
from collections import defaultdict

import numpy as np
import torch

from . import ops
from .cur import ANCHOR_SELECTIONS, CURApprox, CURRowIndex, select_anchor_items
from .eval_utils import flatten_overlap, overlap_stats_from_counts
from .retrieval import POOL_PREFIX, overlap_pool_cells, pool_cell_limit, split_pool_cells

LOGGER = logging.getLogger(__name__)


def load_score_pickle(path):
	"""The reference's input schema (producer: eval/run_cross_encoder_for_ment_ent_matrix_zeshel.py:230-240)."""
	with open(path, "rb") as f:
		d = pickle.load(f)
	if "ment_to_ent_scores" not in d:
		raise KeyError(f"{path}: not a mention x entity score dump (missing 'ment_to_ent_scores')")
	return d


def load_embeds(path):
	"""Precomputed embeddings of bienc / tfidf: .npy -> a dense NumPy array; .npz in the layout of scipy.sparse.save_npz (keys indptr, indices,
	data, shape, format = csr) -> ops.SparseCSR of host tensors, read with numpy.load alone and checked for canonical form."""
	if not str(path).endswith(".npz"):
		return np.load(path)
	with np.load(path, allow_pickle=False) as z:
		missing = [key for key in ("indptr", "indices", "data", "shape") if key not in z.files]
		if missing:
			raise KeyError(f"{path}: not a scipy.sparse.save_npz file (missing {', '.join(missing)})")
		fmt = z["format"].item() if "format" in z.files else b"csr"
		fmt = fmt.decode("ascii") if isinstance(fmt, bytes) else str(fmt)
		if fmt != "csr":
			raise ValueError(f"{path}: sparse format {fmt}, CSR is required (tocsr() before save_npz)")
		indptr, indices, data, shape = z["indptr"], z["indices"], z["data"], tuple(int(s) for s in z["shape"])
	if indptr.dtype.kind not in "iu" or indices.dtype.kind not in "iu" or data.dtype.kind != "f":
		raise TypeError(f"{path}: indptr / indices must be integer arrays and data a floating-point array")
	return ops.sparse_csr(ops.SparseCSR(torch.from_numpy(indptr.astype(np.int64)), torch.from_numpy(indices.astype(np.int32)),
										torch.from_numpy(data.astype(np.float32)), shape[0], shape[1]), shape[1], str(path))


def take_embed_rows(embeds, rows):
	"""embeds[rows] for a dense array or an ops.SparseCSR on the host (tfidf: the test mentions of all mentions' embeddings, splits.py:378)."""
	rows = np.asarray(rows, dtype=np.int64)
	if not isinstance(embeds, ops.SparseCSR):
		return embeds[rows]
	indptr = embeds.indptr.cpu().numpy()
	counts = (indptr[1:] - indptr[:-1])[rows]
	new_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
	src = torch.from_numpy(np.repeat(indptr[rows] - new_ptr[:-1], counts) + np.arange(new_ptr[-1], dtype=np.int64))
	return ops.SparseCSR(torch.from_numpy(new_ptr), embeds.indices.cpu()[src], embeds.data.cpu()[src], rows.size, embeds.n_cols)


def to_device_matrix(scores, device, dtype="fp32"):
	t = scores if torch.is_tensor(scores) else torch.as_tensor(np.asarray(scores))
	t = t.to(device=device, dtype=torch.float32)
	return ops.convert(t, torch.bfloat16) if dtype == "bf16" else t.contiguous()


def _select(rng, n, size):
	"""sorted(rng.choice(n, size, replace=False)) -- the reference's anchor selection (crossenc.py:67-68, splits.py:295)."""
	return sorted(rng.choice(n, size=size, replace=False))


def _subset_metrics(counts_row, rows, k, prefix=None):
	stats = overlap_stats_from_counts(np.asarray(counts_row)[np.asarray(rows, dtype=np.int64)], k)
	return flatten_overlap(stats) if prefix is None else flatten_overlap(stats, prefix=prefix)


RERANK_POOLS = ("retrieved", "retrieved+anchors")   # --rerank_pool of both entry points


def _check_rerank_pool(rerank_pool):
	if rerank_pool not in RERANK_POOLS:
		raise ValueError(f"rerank_pool = {rerank_pool} not supported (one of {', '.join(RERANK_POOLS)})")
	return rerank_pool == "retrieved+anchors"


def _log_skipped_pool_cells(skipped, n_anc, n_ent):
	LOGGER.info("rerank_pool=retrieved+anchors: %d cell(s) with %d anchor items left out of %s (k_retvr %s): k_retvr + n_anc exceeds min(n_ent, ANNCUR_MAX_TOPK, %d) = %d, "
				"what one retrieval with the anchors excluded and one overlap list hold", len(skipped), n_anc, POOL_PREFIX,
				",".join(str(kr) for kr in sorted({c[1] for c in skipped})), 4096, pool_cell_limit(n_ent))


# ------------------------------------------------------------------------------------------------ entry point A
def run_approx_eval_w_seed(approx_method, A_dev, n_ment_anchors, n_ent_anchors, top_k, top_k_retvr, seed, exact_cache=None, pinv_backend="auto", compute_dtype=None,
						   rerank_pool="retrieved", literal_rerank=False, pinv_rcond=None):
	"""One seed of one grid cell -> {"anchor": {...}, "non_anchor": {...}, "all": {...}} (crossenc.py:47-158).
	compute_dtype: CURApprox's (None = by the matrix' dtype; "bf16x3" = the fp32-parity route on the bf16 matrix cores).
	rerank_pool "retrieved+anchors": every subset also reports the overlap metrics of the pool anchor items + top_k_retvr NEW items under
	POOL_PREFIX (a second retrieval, with the anchor items excluded); a cell beyond pool_cell_limit is left out of that prefix.
	pinv_rcond: CURApprox's rcond= (pinv_backend "svd" / "numpy": the cutoff of pinv(W); None = the reference's 1e-15, today's call)."""
	with_pool = _check_rerank_pool(rerank_pool)
	rcond_kw = {} if pinv_rcond is None else {"rcond": pinv_rcond}
	n_ments, n_ents = A_dev.shape
	rng = np.random.default_rng(seed=seed)
	row_idxs = _select(rng, n_ments, n_ment_anchors)          # rows first, then columns, same generator
	col_idxs = _select(rng, n_ents, n_ent_anchors)
	rows = ops.gather_rows(A_dev, row_idxs)
	cols = ops.gather_cols(A_dev, col_idxs)
	non_anchor = sorted(set(range(n_ments)) - set(int(i) for i in row_idxs))
	if approx_method == "cur":
		cur = CURApprox(rows=rows, cols=cols, row_idxs=row_idxs, col_idxs=col_idxs, approx_preference="rows", pinv_backend=pinv_backend, compute_dtype=compute_dtype, **rcond_kw)
	elif approx_method == "cur_oracle":
		cur = CURApprox(rows=rows, cols=cols, row_idxs=row_idxs, col_idxs=col_idxs, approx_preference="rows", A=A_dev, pinv_backend=pinv_backend, compute_dtype=compute_dtype, **rcond_kw)
	else:
		raise NotImplementedError(f"approx_method = {approx_method} not supported")
	# approximate retrieval for EVERY query row + the per-row error terms: one sweep where the fused route takes the cell (cur.eval_rows)
	approx, err_sq, norm_sq = cur.eval_rows(cols, A_dev, top_k_retvr)
	if exact_cache is not None and exact_cache.get("k", 0) >= top_k:
		exact = exact_cache["topk"]
	else:
		exact = ops.rowwise_topk(A_dev, top_k)
		if exact_cache is not None:
			exact_cache.update(k=top_k, topk=exact)
	counts = ops.overlap_counts(exact.indices, approx.indices, [(top_k, top_k_retvr)]).cpu().numpy()[0]
	err_sq, norm_sq = err_sq.double().cpu().numpy(), norm_sq.double().cpu().numpy()
	pool_counts = None
	if with_pool:
		cell = [(top_k, top_k_retvr)]
		kept, skipped = split_pool_cells(cell, n_ent_anchors, n_ents)
		if skipped:
			_log_skipped_pool_cells(skipped, n_ent_anchors, n_ents)
		else:
			new_items = cur.topk_in_row_device(cols, top_k_retvr, exclude=np.asarray(col_idxs))
			pool_counts = overlap_pool_cells(exact.indices, col_idxs, new_items.indices, kept, A_dev, literal_rerank).cpu().numpy()[0]

	def score(idxs):
		res = _subset_metrics(counts, idxs, top_k) if len(idxs) else flatten_overlap(overlap_stats_from_counts([], top_k))
		if pool_counts is not None:
			res.update(_subset_metrics(pool_counts, idxs, top_k, POOL_PREFIX) if len(idxs) else flatten_overlap(overlap_stats_from_counts([], top_k), prefix=POOL_PREFIX))
		ii = np.asarray(idxs, dtype=np.int64)
		err = np.float32(np.sqrt(err_sq[ii].sum()))
		with np.errstate(invalid="ignore", divide="ignore"):
			res["approx_error"] = err
			res["approx_error_relative"] = err / np.float32(np.sqrt(norm_sq[ii].sum()))  # empty subset -> 0/0 = nan, like the reference
		return res

	return {"anchor": score(row_idxs), "non_anchor": score(non_anchor), "all": score(list(range(n_ments)))}


def run_approx_eval(approx_method, A_dev, n_ment_anchors, n_ent_anchors, top_k, top_k_retvr, n_seeds, exact_cache=None, pinv_backend="auto", compute_dtype=None,
					rerank_pool="retrieved", literal_rerank=False, pinv_rcond=None):
	"""Mean over seeds (crossenc.py:162-200)."""
	acc = defaultdict(lambda: defaultdict(list))
	for seed in range(n_seeds):
		res = run_approx_eval_w_seed(approx_method, A_dev, n_ment_anchors, n_ent_anchors, top_k, top_k_retvr, seed, exact_cache, pinv_backend, compute_dtype,
									 rerank_pool=rerank_pool, literal_rerank=literal_rerank, **({} if pinv_rcond is None else {"pinv_rcond": pinv_rcond}))
		for ment_type, d in res.items():
			for metric, val in d.items():
				acc[ment_type][metric].append(float(val))
	return {t: {m: float(np.mean(v)) for m, v in d.items()} for t, d in acc.items()}


def run_approx_eval_w_seed_sharded(sharded, n_ment_anchors, n_ent_anchors, top_k, top_k_retvr, seed):
	"""Method "cur" of entry point A on a ROW-SHARDED score matrix (anncur_amd.dist.ShardedScoreMatrix): every rank holds a
	contiguous block of query rows.  One all-gather assembles the anchor rows; the index is replicated; each rank retrieves,
	scans and counts for its own rows; rank 0 receives the ordered per-query counts / error terms and returns the same dict as
	run_approx_eval_w_seed (None on the other ranks).  No collective on the per-query path."""
	from .dist import gather_rows_to_rank0
	A_loc, n_ments = sharded.local, sharded.n_rows
	n_ents = A_loc.shape[1]
	rng = np.random.default_rng(seed=seed)
	row_idxs = _select(rng, n_ments, n_ment_anchors)
	col_idxs = _select(rng, n_ents, n_ent_anchors)
	R = sharded.anchor_rows(row_idxs)                                  # the one exchange: [Kq x I] on every rank
	index = CURRowIndex(R, col_idxs)
	X_loc = ops.gather_cols(A_loc, col_idxs)
	exact, approx, err_sq, norm_sq = index.eval_cell(X_loc, A_loc, top_k, top_k_retvr)   # exact scan beside ONE sweep for candidates + error sums
	counts = ops.overlap_counts(exact.indices, approx.indices, [(top_k, top_k_retvr)])[0]
	packed = torch.stack([counts.float(), err_sq, norm_sq], dim=1).contiguous()      # [n_loc x 3]
	full = gather_rows_to_rank0(packed, n_ments, sharded.group)
	if full is None:
		return None
	full = full.double().cpu().numpy()
	counts_all, err_all, norm_all = full[:, 0].round().astype(np.int64), full[:, 1], full[:, 2]
	non_anchor = sorted(set(range(n_ments)) - set(int(i) for i in row_idxs))

	def score(idxs):
		res = _subset_metrics(counts_all, idxs, top_k) if len(idxs) else flatten_overlap(overlap_stats_from_counts([], top_k))
		ii = np.asarray(idxs, dtype=np.int64)
		err = np.float32(np.sqrt(err_all[ii].sum()))
		with np.errstate(invalid="ignore", divide="ignore"):
			res["approx_error"] = err
			res["approx_error_relative"] = err / np.float32(np.sqrt(norm_all[ii].sum()))
		return res

	return {"anchor": score(row_idxs), "non_anchor": score(non_anchor), "all": score(list(range(n_ments)))}


def run_entry_A_sharded(sharded, grids, n_seeds, progress=None):
	"""run_entry_A for a row-sharded matrix (method "cur" only: "cur_oracle" needs the whole matrix on one device).
	Rank 0 returns the result dict, the other ranks None."""
	from .dist import dist
	is_root = dist.get_rank(sharded.group) == 0
	n_ment, n_ent = sharded.n_rows, sharded.local.shape[1]
	res = defaultdict(lambda: defaultdict(lambda: defaultdict(dict)))
	cells = list(itertools.product(grids["top_k_vals"], grids["top_k_retr_vals"], grids["n_ment_anchors_vals"], grids["n_ent_anchors_vals"]))
	for ctr, (top_k, kr, nm, ne) in enumerate(cells):
		if kr < top_k or kr > n_ent or nm > n_ment or ne > n_ent:
			continue
		if progress and is_root:
			progress("cur", ctr, len(cells))
		acc = defaultdict(lambda: defaultdict(list))
		for seed in range(n_seeds):
			out = run_approx_eval_w_seed_sharded(sharded, nm, ne, top_k, kr, seed)
			if is_root:
				for ment_type, d in out.items():
					for metric, val in d.items():
						acc[ment_type][metric].append(float(val))
		if is_root:
			res["cur"][f"top_k={top_k}"][f"k_retvr={kr}"][f"anc_n_m={nm}~anc_n_e={ne}"] = \
				{t: {m: float(np.mean(v)) for m, v in d.items()} for t, d in acc.items()}
	if not is_root:
		return None
	return {m: {a: {b: dict(c) for b, c in d.items()} for a, d in v.items()} for m, v in res.items()}


def default_grids_A(total_n_ment, total_n_ent):
	"""The grids hard-coded in the reference (crossenc.py:225-239)."""
	return {
		"eval_methods": ["cur", "cur_oracle"],
		"n_ment_anchors_vals": [v for v in [50, 100, 200, 500, 1000, 2000, 5000] if v <= total_n_ment],
		"n_ent_anchors_vals": [v for v in [50, 100, 200, 500, 1000, 2000] if v < total_n_ent] + [total_n_ent],
		"top_k_vals": [10],
		"top_k_retr_vals": [500],
	}


def run_entry_A(A_dev, grids, n_seeds, progress=None, pinv_backend="auto", compute_dtype=None, rerank_pool="retrieved", literal_rerank=False, pinv_rcond=None):
	"""-> res[method]["top_k=.."]["k_retvr=.."]["anc_n_m=..~anc_n_e=.."][anchor|non_anchor|all][metric]  (crossenc.py:349-383)."""
	total_n_ment, total_n_ent = A_dev.shape
	res = defaultdict(lambda: defaultdict(lambda: defaultdict(dict)))
	exact_cache = {}
	for method in grids["eval_methods"]:
		cells = list(itertools.product(grids["top_k_vals"], grids["top_k_retr_vals"], grids["n_ment_anchors_vals"], grids["n_ent_anchors_vals"]))
		for ctr, (top_k, kr, nm, ne) in enumerate(cells):
			if kr < top_k or kr > total_n_ent:     # crossenc.py:358-359
				continue
			if nm > total_n_ment or ne > total_n_ent:
				continue
			if progress:
				progress(method, ctr, len(cells))
			res[method][f"top_k={top_k}"][f"k_retvr={kr}"][f"anc_n_m={nm}~anc_n_e={ne}"] = \
				run_approx_eval(method, A_dev, nm, ne, top_k, kr, n_seeds, exact_cache, pinv_backend, compute_dtype, rerank_pool=rerank_pool, literal_rerank=literal_rerank,
								**({} if pinv_rcond is None else {"pinv_rcond": pinv_rcond}))
	return {m: {a: {b: dict(c) for b, c in d.items()} for a, d in v.items()} for m, v in res.items()}


# ------------------------------------------------------------------------------------------------ entry point B
def default_grids_B(total_n_ent, method="cur"):
	"""The grids hard-coded in the reference (splits.py:238-251)."""
	base = [1, 10, 50, 100, 200, 500, 1000]
	cur = base + [int(k * frac) for k in base for frac in np.arange(0.1, 1.0, 0.1)]
	retr = cur if ("cur" in method or "fixed_anc_ent" in method) else base
	n_anc = [v for v in [10, 50, 100, 200, 500, 1000, 2000] if v < total_n_ent] + [total_n_ent]
	return {"top_k_vals": [1, 10, 50, 100], "top_k_retr_vals": sorted(set(retr)), "n_ent_anchors_vals": sorted(set(n_anc + cur))}


def _sweep_cells(A_test_dev, approx_idx, exact, top_k_vals, top_k_retr_vals, n_ent):
	"""All (top_k, k_retvr) cells of one approximation from ONE retrieval at the largest k_retvr:
	the top-k_retvr list is a prefix of the sorted top-k_max list."""
	cells = [(k, kr) for kr in top_k_retr_vals if 0 < kr <= n_ent and kr <= approx_idx.shape[1] for k in top_k_vals if k <= kr]
	if not cells:
		return {}
	counts = ops.overlap_counts(exact.indices, approx_idx, cells).cpu().numpy()
	return {cell: flatten_overlap(overlap_stats_from_counts(counts[j], cell[0])) for j, cell in enumerate(cells)}


def _sweep_pool_cells(A_test_dev, anc, retrieved_idx, exact, top_k_vals, top_k_retr_vals, n_ent, literal_rerank=False):
	"""The pool-mode metrics (POOL_PREFIX) of all (top_k, k_retvr) cells of one anchor set from ONE retrieval with the anchors excluded, at the
	largest k_retvr the pool takes: the pool of a cell is the anchor items + the first k_retvr retrieved.  Cells beyond pool_cell_limit
	are left out, with one log line."""
	cells = [(k, kr) for kr in top_k_retr_vals if 0 < kr <= min(n_ent, ops._lib.MAX_TOPK) for k in top_k_vals if k <= kr and k <= exact.indices.shape[1]]
	kept, skipped = split_pool_cells(cells, len(anc), n_ent)
	if skipped:
		_log_skipped_pool_cells(skipped, len(anc), n_ent)
	kept = [c for c in kept if c[1] <= retrieved_idx.shape[1]]
	if not kept:
		return {}
	counts = overlap_pool_cells(exact.indices, anc, retrieved_idx, kept, A_test_dev, literal_rerank).cpu().numpy()
	return {cell: flatten_overlap(overlap_stats_from_counts(counts[j], cell[0]), prefix=POOL_PREFIX) for j, cell in enumerate(kept)}


def _pivoted_anchor_counts(A_train_dev, anc_vals):
	"""anchor_selection "pivoted": ONE select_anchor_items call at the largest anchor count the selection can deliver -- n_anc <= the number
	of training queries kq (a column of R has kq entries: no more directions exist), <= ANNCUR_MAX_TOPK and <= the numerical rank n_sel it
	stops at -- serves every count (the selection is nested).  -> (AnchorSelection or None, the counts left out); those are logged once."""
	kq, n_ent = A_train_dev.shape
	lim = min(kq, n_ent, ops._lib.MAX_TOPK)
	usable = [n for n in anc_vals if 0 < n <= lim]
	sel = select_anchor_items(A_train_dev, max(usable), method="pivoted") if usable else None
	skipped = sorted({n for n in anc_vals if n > 0 and (n > lim or n > sel.n_sel)})
	if skipped:
		LOGGER.info("anchor_selection=pivoted: %d anchor count(s) left out (n_ent_anchors %s): the selection delivers at most min(kq, n_ent, ANNCUR_MAX_TOPK) = "
					"min(%d, %d, %d) = %d items and stopped at the numerical rank n_sel = %s", len(skipped), ",".join(str(n) for n in skipped), kq, n_ent,
					ops._lib.MAX_TOPK, lim, "-" if sel is None else sel.n_sel)
	return sel, skipped


ADAPTIVE_PREFIX = "exact_vs_reranked_adaptive_retvr"   # --adaptive_rounds of entry point B
ADAPTIVE_SOFTMAX_PREFIX = "exact_vs_reranked_adaptive_softmax_retvr"   # ... with --adaptive_strategy softmax


def _sweep_adaptive_cells(A_test_dev, A_train_dev, anc, exact, top_k_vals, top_k_retr_vals, n_rounds, compute_dtype, pinv_backend, incremental=False,
						  strategy="topk", temperature=1.0, seed=0, pinv_rcond=None):
	"""The adaptive-search metrics (ADAPTIVE_PREFIX) of the (top_k, k_retvr) cells of one anchor set: the pool of a cell is the anchor items
	+ n_rounds rounds of k_retvr / n_rounds NEW items each, scored through MatrixScorer(A_test) -- its own AdaptiveSearcher run per k_retvr,
	because adaptive results are not prefixes of one another --, and recall is the closed form |exact[:k] & pool| (retrieval.overlap_pool_cells'
	statement: one ops.overlap_counts call on the pool's id list).  Cells with k_retvr % n_rounds != 0 or outside search.adaptive_limits
	are left out, with one log line for the anchor set that names the limit.  incremental: AdaptiveSearcher's switch (the per-query factorisation
	extended round by round), with its own limit kc + (n_rounds - 1) k_step <= kq among those.  strategy / temperature / seed: AdaptiveSearcher's
	(DESIGN 4.4e); "softmax" cells report under ADAPTIVE_SOFTMAX_PREFIX, so the two strategies' files can be merged."""
	from .search import AdaptiveSearcher, MatrixScorer, adaptive_limits
	prefix = ADAPTIVE_SOFTMAX_PREFIX if strategy == "softmax" else ADAPTIVE_PREFIX
	out, skipped = {}, []
	if len(anc) == 0:
		LOGGER.info("adaptive_rounds=%d: no anchor items: every cell left out of %s (the first round needs anchor scores)", n_rounds, prefix)
		return out
	index = CURRowIndex(A_train_dev, np.asarray(anc), compute_dtype=compute_dtype, pinv_backend=pinv_backend, **({} if pinv_rcond is None else {"rcond": pinv_rcond}))
	searcher = AdaptiveSearcher(index, MatrixScorer(A_test_dev), incremental=incremental, strategy=strategy, temperature=temperature, seed=seed)
	qids = torch.arange(A_test_dev.shape[0], dtype=torch.int64)
	for kr in top_k_retr_vals:
		ks = [k for k in top_k_vals if k <= kr and k <= exact.indices.shape[1]]
		if kr <= 0 or not ks:
			continue
		if kr % n_rounds:
			skipped.append((kr, f"k_retvr % {n_rounds} != 0"))
			continue
		try:
			adaptive_limits(searcher.kc, searcher.kq, index.m, 1, kr // n_rounds, n_rounds, incremental)
		except ValueError as e:
			skipped.append((kr, str(e)))
			continue
		pool = searcher.search(qids, 1, kr // n_rounds, n_rounds, trace=True).trace[-1]["ids"]      # the final S_q: anchors + everything scored
		counts = ops.overlap_counts(exact.indices, pool, [(k, pool.shape[1]) for k in ks]).cpu().numpy()
		for j, k in enumerate(ks):
			out[(k, kr)] = flatten_overlap(overlap_stats_from_counts(counts[j], k), prefix=prefix)
	if skipped:
		LOGGER.info("adaptive_rounds=%d: %d k_retvr value(s) with %d anchor items left out of %s: %s", n_rounds, len(skipped), len(anc), prefix,
					"; ".join(f"k_retvr={kr}: {why}" for kr, why in skipped))
	return out


RANK_METRICS_KEY = "approx_rank"   # --rank_metrics of entry point B: res["top_k=k"][RANK_METRICS_KEY]["anc_n_m=.._anc_n_e=.."]


def _put_rank_metrics(res, ranks, top_k_vals, k_max, anc_key):
	"""ranks [Q x k_max]: the approximate ranks of the exact top-k_max items, in exact order."""
	from .retrieval import rank_curve
	for k, metrics in rank_curve(ranks, [k for k in top_k_vals if k <= k_max]).items():
		res[f"top_k={k}"][RANK_METRICS_KEY][anc_key] = metrics


def run_eval_method_cur(A_test_dev, A_train_dev, seed, grids, compute_dtype=None, progress=None, key_n_m=None, pinv_backend="auto", rerank_pool="retrieved",
						literal_rerank=False, adaptive_rounds=1, adaptive_incremental=False, adaptive_strategy="topk", adaptive_temperature=1.0, adaptive_seed=0,
						anchor_selection="random", rank_metrics=False, pinv_rcond=None):
	"""eval_method == "cur" of entry point B for one seed (splits.py:286-303 + 399-429).
	rerank_pool "retrieved+anchors": every cell also reports, under POOL_PREFIX, the metrics of the pool anchor items + k_retvr NEW items (a
	second retrieval per anchor count, with the anchor items excluded, at the largest k_retvr with k_retvr + n_anc <= pool_cell_limit).
	adaptive_rounds N >= 2: every cell with k_retvr divisible by N also reports, under ADAPTIVE_PREFIX, the metrics of the adaptive search's
	pool at the same budget (_sweep_adaptive_cells); 1 is today's code path.  adaptive_incremental: that search with AdaptiveSearcher(incremental=True);
	the output keys are the same.  adaptive_strategy "softmax" (with adaptive_temperature, adaptive_seed): that search with sampled rounds
	(DESIGN 4.4e), reported under ADAPTIVE_SOFTMAX_PREFIX instead.
	anchor_selection "random": the reference's sorted(rng.choice(...)) per anchor count, today's code path and rng stream.  "pivoted" (DESIGN
	4.4f): the anchor items of every count are the sorted first n_anc of ONE column-pivoted QR selection from A_train; `seed` is not used,
	counts the selection cannot deliver are left out and logged once (_pivoted_anchor_counts), n_anc = 0 keeps its branch; the pool and
	adaptive modes see only the anchor list.
	pinv_rcond: the rcond= of every index built here (pinv_backend "svd" / "numpy": the cutoff of pinv(W); None = the reference's 1e-15, today's call).
	rank_metrics (--rank_metrics; with adaptive_rounds 1): every top_k also reports, under res["top_k=k"]["approx_rank"]["anc_n_m=.._anc_n_e=.."],
	retrieval.rank_curve of the approximate ranks of the exact top-k items -- one cur.rank_in_row call per anchor count: the whole
	recall curve, beyond ANNCUR_MAX_TOPK too, and the smallest k_retvr that reaches a recall."""
	with_pool = _check_rerank_pool(rerank_pool)
	rcond_kw = {} if pinv_rcond is None else {"rcond": pinv_rcond}
	if rank_metrics and adaptive_rounds != 1:
		raise ValueError(f"rank_metrics needs adaptive_rounds = 1 (got {adaptive_rounds}): an adaptive pool is no prefix of one ranking")
	if anchor_selection not in ANCHOR_SELECTIONS:
		raise ValueError(f"anchor_selection = {anchor_selection} not supported (one of {', '.join(ANCHOR_SELECTIONS)})")
	if adaptive_rounds < 1:
		raise ValueError(f"adaptive_rounds = {adaptive_rounds}: need adaptive_rounds >= 1")
	n_train, n_ent = A_train_dev.shape
	top_k_vals, retr_vals, anc_vals = grids["top_k_vals"], grids["top_k_retr_vals"], grids["n_ent_anchors_vals"]
	kr_max = max([kr for kr in retr_vals if kr <= min(n_ent, ops._lib.MAX_TOPK)] or [0])
	k_max = max([k for k in top_k_vals if k <= kr_max] or [0])
	if kr_max == 0 or k_max == 0:
		return {}
	exact = ops.rowwise_topk(A_test_dev, k_max)
	rng = np.random.default_rng(seed=seed)                     # ONE stream consumed across the whole anchor-count loop
	res = defaultdict(lambda: defaultdict(dict))
	pivoted, left_out = _pivoted_anchor_counts(A_train_dev, anc_vals) if anchor_selection == "pivoted" else (None, ())
	for j, n_anc in enumerate(anc_vals):
		if n_anc in left_out:
			continue
		anc = _select(rng, n_ent, n_anc) if anchor_selection == "random" else (pivoted.sorted(n_anc) if n_anc else [])
		if progress:
			progress(j, len(anc_vals))
		if n_anc == 0:
			# the reference's own grid holds n_ent_anchors = int(1 * 0.1) = 0 (splits.py:241,250): C is [n x 0], U = pinv of an
			# empty block, S_hat = 0 everywhere.  Every item ties; under this build's tie order (score desc, index asc) the
			# retrieved list is 0..k_retvr-1 for every query (torch.topk leaves the order of an all-equal row unspecified).
			approx_idx = torch.arange(kr_max, dtype=torch.int32, device=A_test_dev.device).expand(A_test_dev.shape[0], kr_max).contiguous()
			for (k, kr), metrics in _sweep_cells(A_test_dev, approx_idx, exact, top_k_vals, retr_vals, n_ent).items():
				res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}"] = metrics
			if rank_metrics:   # (every score ties: an item's rank is its id)
				_put_rank_metrics(res, exact.indices, top_k_vals, k_max, f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}")
			if with_pool:   # no anchors: the pool is the retrieved list
				for (k, kr), metrics in _sweep_pool_cells(A_test_dev, anc, approx_idx, exact, top_k_vals, retr_vals, n_ent, literal_rerank).items():
					res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}"].update(metrics)
			continue
		cur = CURApprox(rows=A_train_dev, cols=ops.gather_cols(A_train_dev, anc), row_idxs=np.arange(n_train), col_idxs=anc,
						approx_preference="rows", compute_dtype=compute_dtype, pinv_backend=pinv_backend, **rcond_kw)
		X = ops.gather_cols(A_test_dev, anc)
		approx = cur.topk_in_row_device(X, kr_max)
		for (k, kr), metrics in _sweep_cells(A_test_dev, approx.indices, exact, top_k_vals, retr_vals, n_ent).items():
			res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}"] = metrics
		if rank_metrics:
			ranks = torch.cat([cur.rank_in_row(X, exact.indices[:, c:c + ops.RANK_MAX_T]) for c in range(0, k_max, ops.RANK_MAX_T)], dim=1)
			_put_rank_metrics(res, ranks, top_k_vals, k_max, f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}")
		if with_pool:
			kr_pool = max([kr for kr in retr_vals if 0 < kr and kr + n_anc <= pool_cell_limit(n_ent)] or [0])
			new_items = cur.topk_in_row_device(X, kr_pool, exclude=np.asarray(anc)).indices if kr_pool else approx.indices[:, :0]
			for (k, kr), metrics in _sweep_pool_cells(A_test_dev, anc, new_items, exact, top_k_vals, retr_vals, n_ent, literal_rerank).items():
				res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}"].update(metrics)
			del new_items
		if adaptive_rounds >= 2:
			for (k, kr), metrics in _sweep_adaptive_cells(A_test_dev, A_train_dev, anc, exact, top_k_vals, retr_vals, adaptive_rounds, compute_dtype, pinv_backend,
																  adaptive_incremental, adaptive_strategy, adaptive_temperature, adaptive_seed,
																  **({} if pinv_rcond is None else {"pinv_rcond": pinv_rcond})).items():
				res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train if key_n_m is None else key_n_m}_anc_n_e={n_anc}"].update(metrics)
		del cur, approx
	return {a: {b: dict(c) for b, c in d.items()} for a, d in res.items()}


def run_eval_method_embeds(A_test_dev, mention_embeds, label_embeds, n_train, grids):
	"""bienc / tfidf / fixed_anc_ent given PRECOMPUTED embeddings: scores = mention_embeds @ label_embeds.T (splits.py:283,324,383);
	one result is repeated for every anchor count, as the reference does (splits.py:412-418).
	Sparse embeddings (tfidf: CSR objects or ops.SparseCSR, see ops.is_sparse_arg) are retrieved through the term-major index instead of
	being densified; if only one side is sparse, the dense side is sparsified."""
	sparse = ops.is_sparse_arg(mention_embeds) or ops.is_sparse_arg(label_embeds)
	if sparse:
		dims = [int(e.shape[1]) if hasattr(e, "shape") else getattr(e, "n_cols", None) for e in (label_embeds, mention_embeds)]
		mention_embeds, label_embeds = (e if ops.is_sparse_arg(e) else ops.sparse_from_dense(e) for e in (mention_embeds, label_embeds))
		label_embeds = ops.sparse_csr(label_embeds, dims[0] if dims[0] is not None else dims[1], "label_embeds")   # (a bare triple takes the other side's width)
		n_ent = label_embeds.n_rows
	else:
		n_ent = label_embeds.shape[0]
	top_k_vals, retr_vals, anc_vals = grids["top_k_vals"], grids["top_k_retr_vals"], grids["n_ent_anchors_vals"]
	kr_max = max([kr for kr in retr_vals if kr <= min(n_ent, ops._lib.MAX_TOPK)] or [0])
	k_max = max([k for k in top_k_vals if k <= kr_max] or [0])
	if kr_max == 0:
		return {}
	exact = ops.rowwise_topk(A_test_dev, k_max)
	if sparse:
		approx = ops.sparse_score_topk(mention_embeds, ops._postings_of(label_embeds, A_test_dev.device), kr_max)
	else:
		approx = ops.score_topk_dense(mention_embeds, label_embeds, kr_max)
	res = defaultdict(lambda: defaultdict(dict))
	for (k, kr), metrics in _sweep_cells(A_test_dev, approx.indices, exact, top_k_vals, retr_vals, n_ent).items():
		for n_anc in anc_vals:
			res[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train}_anc_n_e={n_anc}"] = metrics
	return {a: {b: dict(c) for b, c in d.items()} for a, d in res.items()}


def run_eval_method_fixed_anc_ent_cur(A_test_dev, e2e_scores_dev, n_fixed_anc_ent, grids, key_n_m=None, rerank_pool="retrieved"):
	"""fixed_anc_ent_cur (splits.py:327-358): R = ent_to_ent_scores[:, :n_fixed].T, anchors from rng(0), U = pinv(R[:, anc])."""
	R = e2e_scores_dev[:, :n_fixed_anc_ent].t().contiguous()     # n_fixed x n_ents
	return run_eval_method_cur(A_test_dev, R, seed=0, grids=grids, key_n_m=key_n_m, rerank_pool=rerank_pool)
