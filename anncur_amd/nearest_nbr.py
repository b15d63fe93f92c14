"""Flat exact inner-product index with the FAISS calling convention the reference relies on
(models/nearest_nbr.py:24-55; call sites utils/data_process.py:343-351,393-397 and
eval/run_cross_encoder_w_binenc_retriever_zeshel.py:125,147):

    index = build_flat_or_ivff_index(embeds, force_exact_search)
    D, I = index.search(queries, k)      # D float32 [nq, k] descending, I int64 [nq, k]   (NumPy, like FAISS)

FAISS itself is a third-party dependency that the reference neither vendors nor pins: parity at this boundary is UNPINNED and
judged against torch.topk(q @ X^T) (tests/).  Like the reference, up to 11 000 vectors (or with force_exact_search) the index is
flat and exact; above, it is an IVF-flat index with nlist = floor(sqrt(n)) lists and nprobe = floor(sqrt(nlist) * probe_mult_factor)
probed lists (models/nearest_nbr.py:40-52), built and searched on the GPU (IVFFlatIPIndex), judged on recall against the exact search.
"""
import logging
import math

import numpy as np
import torch

from . import ops

LOGGER = logging.getLogger(__name__)


PAD_SCORE = np.float32(np.finfo(np.float32).min)   # -FLT_MAX: the neutral element of FAISS' inner-product result heaps (CMin<float>::neutral())


def _faiss_pad(v, i, nq, k, k_eff):
	"""(D float32 [nq, k], I int64 [nq, k]) NumPy arrays; slots without a result hold (-FLT_MAX, -1) as FAISS leaves them for
	METRIC_INNER_PRODUCT (the kernels mark them (-inf, -1))."""
	D = np.full((nq, k), PAD_SCORE, dtype=np.float32)
	I = np.full((nq, k), -1, dtype=np.int64)
	I[:, :k_eff] = i.cpu().numpy().astype(np.int64)
	D[:, :k_eff] = np.where(I[:, :k_eff] >= 0, v.cpu().numpy(), PAD_SCORE)
	return D, I


class FlatIPIndex:
	"""Exact maximum-inner-product search on the GPU.  fp32 by default (dense fp32-MFMA GEMM + exact scan);
	dtype="bf16" uses the fused score+top-k kernel when the dimension fits (d <= 4096: the register-resident bodies up to 512, the
	K-general wide kernel above); dtype="bf16x3" keeps fp32 parity on that kernel: the stored fp32 vectors split into bf16 hi + lo
	parts (3 d <= 4096), the fused kernel for the candidates, an fp32 rescore for the values -- those of the fp32 route bit for bit.
	Score ties: the fp32 route orders them by the smaller id; the bf16 route on the fused kernel by the smaller ROW of its descending-norm copy
	(256 norm buckets, id order inside a bucket), so by the smaller id only among vectors of one norm bucket (tests/test_gpu_ivf_index_exact.py)."""

	def __init__(self, d, dtype="fp32", device=None, small_batch=False):
		"""small_batch: dtype "bf16" only -- searches of up to 64 queries take the small-batch route on an item-order packed copy (DESIGN 4.4h;
		search_route names the route of a call; ties by the smaller id there)."""
		self.d = d
		self.dtype = dtype
		self.small_batch = bool(small_batch)
		self._Xp_items = None        # small_batch: packed bf16 copy in item order (built at the first such search)
		self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
		self.ntotal = 0
		self._X = None
		self._Xp = self._ids = None  # packed bf16 copy in descending-norm order + row -> id map (built at the first bf16 search)
		self._split = None           # dtype "bf16x3": the split-bf16 copy (built at the first search)
		self._rank_operand = None    # the item operand of rank() (built at the first call)
		self.nprobe = 1  # accepted for FAISS API compatibility

	def add(self, embeds):
		x = torch.as_tensor(np.ascontiguousarray(embeds, dtype=np.float32)).to(self.device)
		assert x.dim() == 2 and x.shape[1] == self.d, f"expected [n, {self.d}] embeddings"
		self._X = x if self._X is None else torch.cat([self._X, x], dim=0)
		self.ntotal = self._X.shape[0]
		self._Xp = self._Xp_items = self._split = self._rank_operand = None

	def train(self, embeds):  # FAISS API compatibility (flat index needs no training)
		return None

	def search(self, x, k, exclude=None):
		"""exclude: vector ids left out of the result, FAISS' id selector turned round (ops.exclusion: one list for all queries, one per
		query, or a -1 padded [nq x w] array).  k_eff + the longest list may not exceed min(ntotal, MAX_TOPK): ValueError."""
		assert self._X is not None, "index is empty"
		q = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
		k_eff = min(k, self.ntotal)
		kp = ops.padded_k(self.d)
		from .cur import _exclusion_arg, _filtered
		excl, kc = _exclusion_arg(exclude, q.shape[0], self.ntotal, k_eff, self.device)
		if self.dtype == "bf16x3":
			if self._split is None:
				from .cur import _SplitOperands
				self._split = _SplitOperands.build(self._X)
			if self._split.takes(q.shape[0], self.ntotal, k_eff, excl):
				return _faiss_pad(*self._split.topk(q, self._X, k_eff, excl), q.shape[0], k, k_eff)
		if self._few_takes(q.shape[0], kp, kc):
			if self._Xp_items is None:
				self._Xp_items = ops.pack_bf16(self._X, kp, row_multiple=32)
			v, i = ops.score_topk_few(ops.pack_bf16(q, kp), self._Xp_items, self.ntotal, kc)
		elif self.dtype == "bf16" and kp is not None and ops.fused_supported(q.shape[0], self.ntotal, kp, kc):
			if self._Xp is None:
				from .cur import _norm_sorted_pack
				self._Xp, self._ids = _norm_sorted_pack(self._X, kp)   # largest-norm vectors first: the likeliest maximum inner products
			v, i = ops.score_topk_fused(ops.pack_bf16(q, kp), self._Xp, self.ntotal, kc, leading_sample=True, item_ids=self._ids)
		else:
			v, i = ops.score_topk_dense(q, self._X, kc)
		v, i = _filtered(ops.TopK(v, i), excl, k_eff)
		return _faiss_pad(v, i, q.shape[0], k, k_eff)

	def _few_takes(self, nq, kp, kc):
		return (self.small_batch and self.dtype == "bf16" and kp is not None and kc <= min(self.ntotal, ops._lib.MAX_TOPK)
				and ops.score_topk_few_ok(nq, self.ntotal, kp, kc))

	def search_route(self, nq, k, exclude=None):
		"""The route search() takes for nq queries: "bf16x3", "bf16-few" (small_batch=True, nq <= 64), "bf16" (fused sweep) or "dense"."""
		from .cur import _exclusion_arg
		k_eff, kp = min(k, self.ntotal), ops.padded_k(self.d)
		excl, kc = _exclusion_arg(exclude, nq, self.ntotal, k_eff, self.device)
		if self.dtype == "bf16x3":
			if self._split is None:
				from .cur import _SplitOperands
				self._split = _SplitOperands.build(self._X)
			if self._split.takes(nq, self.ntotal, k_eff, excl):
				return "bf16x3"
		if self._few_takes(nq, kp, kc):
			return "bf16-few"
		if self.dtype == "bf16" and kp is not None and ops.fused_supported(nq, self.ntotal, kp, kc):
			return "bf16"
		return "dense"

	def _rank_op(self):
		if self._rank_operand is None:
			from .cur import _RankOperand
			# dtype "bf16": an ITEM-order packed copy (the search's copy is in descending-norm order); "fp32" / "bf16x3": the stored fp32 vectors
			self._rank_operand = _RankOperand(self._X, "bf16" if self.dtype == "bf16" else "fp32")
		return self._rank_operand

	def rank_route(self, t):
		"""The route rank() takes for t ids per query: "bf16" (fused, no score matrix) or "dense"."""
		from .cur import _rank_route_name
		assert self._X is not None, "index is empty"
		return _rank_route_name(self._rank_op(), t)

	def rank(self, x, ids):
		"""The inverse of search(): ids [nq x t] vector ids (-1 = hole) -> int32 [nq x t] (NumPy), the position of each vector in its query's
		result list (inner product descending, ties to the smaller id), -1 for a hole; at most ops.RANK_MAX_T ids per query.  dtype "bf16" with
		d <= 512 ranks under the bf16 scores without a score matrix; "fp32" and "bf16x3" under the fp32 scores of the dense route."""
		assert self._X is not None, "index is empty"
		from .cur import _route_rank
		q = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
		return _route_rank(self._rank_op(), q, ids).cpu().numpy()

	rank_of = rank   # the name CURRowIndex gives the same question (its `rank` is the anchor block's numerical rank)


class SparseIPIndex:
	"""FlatIPIndex for SPARSE vectors (TF-IDF: the reference densifies them, utils/data_process.py:373-397): exact maximum-inner-product
	search through a term-major index on the device (ops.sparse_postings / ops.sparse_score_topk).  add() takes CSR objects
	(anything with .indptr / .indices / .data / .shape, scipy.sparse.csr_matrix among them) or (indptr, indices, data) triples in
	canonical form; search() also takes a dense [nq x d] array, which is sparsified on the way in.  Scores are the ascending-term fp32
	chain; ties go to the smaller id."""

	def __init__(self, d, dtype="fp32", device=None):
		if dtype != "fp32":
			raise ValueError(f"dtype = {dtype} not supported")
		self.d, self.dtype = int(d), dtype
		self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
		self.ntotal = 0
		self.nprobe = 1        # accepted for FAISS API compatibility
		self._parts = []       # SparseCSR pieces in insertion order (where the caller's arrays live)
		self._postings = None  # rebuilt at the first search after an add

	def add(self, csr):
		part = ops.sparse_csr(csr, self.d, "SparseIPIndex.add")
		self._parts.append(part)
		self.ntotal += part.n_rows
		self._postings = None

	def train(self, embeds):  # FAISS API compatibility
		return None

	def _index(self):
		if self._postings is None:
			assert self._parts, "index is empty"
			parts = [ops.SparseCSR(*(a.to(self.device) for a in p[:3]), p.n_rows, p.n_cols) for p in self._parts]
			if len(parts) > 1:
				offs = np.cumsum([0] + [int(p.indices.numel()) for p in parts])
				indptr = torch.cat([parts[0].indptr] + [p.indptr[1:] + int(o) for p, o in zip(parts[1:], offs[1:])])
				merged = ops.SparseCSR(indptr, torch.cat([p.indices for p in parts]), torch.cat([p.data for p in parts]), self.ntotal, self.d)
				self._parts = parts = [merged]
			self._postings = ops.sparse_postings(*parts[0][:3], self.ntotal, self.d, device=self.device)
		return self._postings

	def _queries(self, x):
		if ops.is_sparse_arg(x):
			return x
		q = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
		assert q.dim() == 2 and q.shape[1] == self.d, f"expected [nq, {self.d}] queries"
		return ops.sparse_from_dense(q.to(self.device))

	def search(self, x, k, exclude=None):
		"""exclude: as FlatIPIndex.search.  -> (D float32 [nq x k], I int64 [nq x k]) NumPy arrays, (-FLT_MAX, -1) where k > ntotal."""
		post = self._index()
		k_eff = min(k, self.ntotal)
		v, i = ops.sparse_score_topk(self._queries(x), post, k_eff, exclude=exclude)
		return _faiss_pad(v, i, v.shape[0], k, k_eff)

	def search_route(self, nq, k, exclude=None):
		return "sparse"


class IVFFlatIPIndex:
	"""faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) on the GPU: train (k-means coarse quantiser) / add
	(inverted lists) / search (exact inner products inside the nprobe best lists).  Restated from FAISS' published algorithm and
	defaults: IndexIVF trains its coarse quantiser through Level1Quantizer, whose ClusteringParameters carry niter = 10 (the
	stand-alone Clustering default is 25: pass niter=25 for that), at most 256 training points per centroid, assignment through the
	inner-product quantiser, centroid = mean of its points RENORMALISED TO UNIT L2 NORM (IndexIVF sets cp.spherical = true for
	METRIC_INNER_PRODUCT: fvec_renorm_L2 after every update, and after the re-seeding of empty lists -- with arg-max inner-product
	assignment an unnormalised mean of large-norm points would keep attracting points and the lists would grow unbalanced; spherical=False
	restores the plain means), an empty list re-seeded by splitting a large one.  FAISS' random draws cannot be reproduced, so parity with
	FAISS is unpinned and the index is judged on recall and list balance.  Results are deterministic for a given seed.

	What IS pinned is the algorithm stated here: tests/ivf_index_numpy.py restates train / add / search on the host (train_ref, add_ref,
	search_ref; flat_search_ref for FlatIPIndex' fp32 route), and tests/test_gpu_ivf_index_exact.py holds both classes to it BIT FOR BIT, with no
	tolerance, on integer data in [-8, 8] (n = 1500 .. 4096 and 11 001, d = 16, 24, 64, 130, nlist = 7, 16, 64, 104; FlatIPIndex fp32 on fixed-point
	grid data, bf16 on integers): scores against centroids are ops.gemm's k-ordered fp32 fmaf chain, top-1 / top-nprobe break ties to the smaller
	list, lists are a stable counting sort, a mean is sum * (1.0f / count), the sub-sample is sorted, the split draws one list per empty list
	with weight max(count - 1, 0) and perturbs by 1 +- 2^-10 on alternating columns, renormalisation comes after the split and on the initial
	centroids; add() rebuilds every list from all vectors; the search pads queries with zeros and breaks score ties by vector id (ivf_scan), by
	probe slot then list position (the batched routes); an exclusion list of e ids is filtered from k + e candidates.  94 tests, 6.2 s on an
	MI355X; ten Python mutants of this file and of ops.score_topk_dense each fail named tests (table in the test's docstring).
	ops.renorm_rows, pinned to the bit as well (1.0f / sqrtf(tot) was measured to be correctly rounded on the device): a row whose sum of
	squares is not > 0 -- all zero, a NaN present, every square underflowing -- stays as it is; squares that overflow give tot = inf, inv = 0,
	a row of (signed) zeros; one infinite element becomes NaN, the others zeros; nothing outside the row's n_cols columns is written."""

	def __init__(self, d, nlist, device=None, niter=10, seed=1234, max_points_per_centroid=256, spherical=True, dtype="fp32"):
		self.d, self.nlist = int(d), int(nlist)
		self.spherical = bool(spherical)
		if dtype not in ("fp32", "bf16"):
			raise ValueError(f"dtype = {dtype} not supported")
		self.dtype = dtype                          # "bf16": the batched search scores bf16 copies of the lists and queries on the bf16 matrix cores
		self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
		self.niter, self.seed, self.max_points_per_centroid = niter, seed, max_points_per_centroid
		self.nprobe = 1
		self.batched_from = 256                     # queries per search() call from which the list-grouped MFMA search runs
		self.grouped_call = True                    # batched search through anncur_ivf_search_grouped (False: round 4's sequence of calls)
		self.ntotal = 0
		self.is_trained = False
		self.centroids = None                       # [nlist x d] fp32
		self._X = None                              # vectors in insertion order
		self._Xs = self._offsets = self._ids = None  # vectors in list order (rows zero-padded to a multiple of 16 floats), list bounds, ids
		self._Xs16 = None                            # dtype "bf16": the same rows rounded to bf16 (batched search)
		# row length of the stored vectors / queries, zero padded: a multiple of 16 floats; of 128 elements for bf16 lists (the 128 x 128-tile
		# GEMM of the batched search streams pairs of 64-wide k-tiles)
		self._dp = -(-self.d // 128) * 128 if dtype == "bf16" else -(-self.d // 16) * 16

	def _dev32(self, x):
		x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
		assert x.dim() == 2 and x.shape[1] == self.d, f"expected [n, {self.d}] vectors"
		return x

	def _assign(self, X):
		"""list of every vector = the centroid of maximum inner product (the IndexFlatIP quantiser's top-1)."""
		return ops.score_topk_dense(X, self.centroids, 1).indices[:, 0].contiguous()

	def train(self, x):
		X = self._dev32(x)
		n = X.shape[0]
		if n < self.nlist:
			raise RuntimeError(f"Number of training points ({n}) should be at least as large as number of clusters ({self.nlist})")
		rng = np.random.default_rng(self.seed)
		cap = self.nlist * self.max_points_per_centroid
		if n > cap:                                                # FAISS subsamples the training set
			X = ops.gather_rows(X, np.sort(rng.choice(n, size=cap, replace=False)))
			n = cap
		self.centroids = ops.gather_rows(X, rng.permutation(n)[:self.nlist])   # initial centroids: distinct random training points
		if self.spherical:
			ops.renorm_rows(self.centroids)   # FAISS post-processes the INITIAL centroids too (Clustering::train): the first assignment already runs on unit vectors
		for it in range(self.niter):
			counts, offsets, ids = ops.ivf_build_lists(self._assign(X), self.nlist)
			ops.ivf_list_means(ops.gather_rows(X, ids), offsets, self.centroids)
			self._split_empty(counts.cpu().numpy(), rng)
			if self.spherical:
				ops.renorm_rows(self.centroids)   # (after the split, as FAISS does: the perturbed copies are renormalised too)
		self.is_trained = True

	def _split_empty(self, counts, rng, eps=1.0 / 1024):
		"""An empty list takes over half of a large one: both get that list's centroid, perturbed symmetrically (FAISS'
		split_clusters).  Rows are edited on the host: a handful of d-vectors per iteration at most."""
		empty = np.flatnonzero(counts == 0)
		if empty.size == 0:
			return
		counts = counts.astype(np.float64).copy()
		C = self.centroids.cpu().numpy()
		for ci in empty:
			w = np.maximum(counts - 1.0, 0.0)
			cj = int(rng.choice(self.nlist, p=w / w.sum()))
			sign = np.where(np.arange(self.d) % 2 == 0, 1.0, -1.0).astype(np.float32)
			C[ci] = C[cj] * (1.0 + sign * eps)
			C[cj] = C[cj] * (1.0 - sign * eps)
			counts[ci] = counts[cj] / 2
			counts[cj] -= counts[ci]
		self.centroids.copy_(torch.from_numpy(C))

	def add(self, x):
		assert self.is_trained, "train() first"
		X = self._dev32(x)
		self._X = X if self._X is None else torch.cat([self._X, X], dim=0)
		self.ntotal = self._X.shape[0]
		counts, self._offsets, self._ids = ops.ivf_build_lists(self._assign(self._X), self.nlist)
		self._sizes = counts.cpu().numpy().astype(np.int64)         # list lengths on the host: the batched search's tile worklist
		self._Xs = torch.zeros((self.ntotal, self._dp), dtype=torch.float32, device=self.device)
		self._Xs[:, :self.d] = ops.gather_rows(self._X, self._ids)
		self._Xs16 = ops.convert(self._Xs, torch.bfloat16) if self.dtype == "bf16" else None

	def search_device(self, q, k, profile=None, exclude=None):
		"""search() on DEVICE-RESIDENT queries q [nq x d] fp32 -> (values f32 [nq x k_eff], ids int32 [nq x k_eff]) on the device, no host copy
		(k_eff = min(k, MAX_TOPK); slots without a result hold (-inf, -1)).  What bench.py times as the kernels' own rate.
		exclude: vector ids left out of the result (ops.exclusion).  The probed lists are searched for k_eff + the longest list -- on the
		one-call path up to IVF_GROUPED_MAX_K, on the older paths above --, one filter launch trims the rows; a row whose probed lists
		hold fewer than k_eff allowed vectors ends in (-inf, -1)."""
		k_eff = min(k, ops._lib.MAX_TOPK)
		from .cur import _exclusion_arg, _filtered
		excl, kc = _exclusion_arg(exclude, q.shape[0], self.ntotal, k_eff, self.device)
		return _filtered(self._search_device(q, kc, profile), excl, k_eff)

	def _search_device(self, q, k, profile):
		assert self._Xs is not None, "index is empty"
		nprobe = max(1, min(int(self.nprobe), self.nlist))
		probe = ops.score_topk_dense(q, self.centroids, nprobe).indices        # the nprobe lists of largest <q, centroid>
		if self._dp == self.d:
			qp = q if q.is_contiguous() else q.contiguous()
		else:
			qp = torch.zeros((q.shape[0], self._dp), dtype=torch.float32, device=self.device)
			qp[:, :self.d] = q
		k_eff = min(k, ops._lib.MAX_TOPK)
		if q.shape[0] >= self.batched_from:
			# many queries (hard-negative mining: every mention): pairs grouped by list, each list one MFMA GEMM -- a list's vectors
			# are read once per 64 queries instead of once per query (28 -> ~3 ms for 10^4 queries on 10^5 x 768 vectors)
			if profile is None and self.grouped_call and ops.ivf_search_grouped_ok(k_eff, self.nlist):
				# round 5: the whole batched search behind one library call (packed score rows, 128 x 128 bf16 tiles)
				if self._Xs16 is not None:
					return ops.ivf_search_grouped(self._Xs16, self._offsets, self._ids, self._sizes, ops.convert(qp, torch.bfloat16), probe, k_eff)
				return ops.ivf_search_grouped(self._Xs, self._offsets, self._ids, self._sizes, qp, probe, k_eff)
			return ops.ivf_scan_grouped(self._Xs, self._offsets, self._ids, self._sizes, qp, probe, k_eff, lists_bf16=self._Xs16, profile=profile)
		return ops.ivf_scan(self._Xs, self._offsets, self._ids, qp, probe, k_eff)

	def search(self, x, k, exclude=None):
		assert self._Xs is not None, "index is empty"
		q = self._dev32(x)
		v, i = self.search_device(q, k, exclude=exclude)
		return _faiss_pad(v, i, q.shape[0], k, min(k, ops._lib.MAX_TOPK))


def _build_sparse_index(embeds, force_exact_search, dtype, device, n_terms):
	if hasattr(embeds, "shape"):
		d = int(embeds.shape[1])
	elif isinstance(embeds, ops.SparseCSR):
		d = embeds.n_cols
	elif n_terms is not None:
		d = int(n_terms)
	else:
		ids = embeds[1]
		d = int(ids.max()) + 1 if len(ids) else 0
	index = SparseIPIndex(d, dtype=dtype, device=device)
	LOGGER.info(f"Beginning indexing given {len(embeds.indptr if hasattr(embeds, 'indptr') else embeds[0]) - 1} sparse embeddings")
	index.add(embeds)
	if index.ntotal > 11000 and not force_exact_search:
		LOGGER.info(f"{index.ntotal} sparse vectors: the sparse index has no IVF form, the search stays exact")
	LOGGER.info("Finished indexing given embeddings")
	return index


def build_flat_or_ivff_index(embeds, force_exact_search, probe_mult_factor=1, dtype="fp32", device=None, n_terms=None):
	"""models/nearest_nbr.py:24-55.  dtype: "fp32", "bf16", or "bf16x3" -- the flat index' fp32-parity route on the bf16 matrix cores.
	The IVF lists stay fp32 / bf16: above 11 000 vectors without force_exact_search, dtype="bf16x3" raises the ValueError IVFFlatIPIndex
	raises for a dtype it does not know.
	A CSR object (.indptr / .indices / .data / .shape) or an (indptr, indices, data) triple -- ops.is_sparse_arg -- gives a SparseIPIndex:
	always exact, whatever the number of vectors; a dtype other than "fp32" is that same ValueError.  n_terms: the dimension of a triple
	(default: its largest term id + 1)."""
	if ops.is_sparse_arg(embeds):
		return _build_sparse_index(embeds, force_exact_search, dtype, device, n_terms)
	LOGGER.info(f"Beginning indexing given {len(embeds)} embeddings")
	if type(embeds) is not np.ndarray:
		embeds = embeds.detach().cpu().numpy() if torch.is_tensor(embeds) else np.array(embeds)
	d, n = embeds.shape[1], embeds.shape[0]
	if n <= 11000 or force_exact_search:    # if the number of embeddings is small, don't approximate (models/nearest_nbr.py:36)
		index = FlatIPIndex(d, dtype=dtype, device=device)
		index.add(embeds)
	else:
		nlist = int(math.floor(math.sqrt(n)))                                   # number of quantized cells (:41)
		nprobe = int(math.floor(math.sqrt(nlist) * probe_mult_factor))          # number of the quantized cells to probe (:44)
		index = IVFFlatIPIndex(d, nlist, device=device, dtype=dtype)
		index.train(embeds)
		index.add(embeds)
		index.nprobe = nprobe
	LOGGER.info("Finished indexing given embeddings")
	return index
