"""CURApprox on the MI355X -- same constructor, attributes, methods and error behaviour as
the reference operator (eval/matrix_approx_zeshel.py:19-126), computed by the HIP kernels
behind include/anncur_hip.h.

    M (n x m)  ~=  C (n x kc) . U (kc x kr) . R (kr x m)

Differences from the reference, all deliberate:
  * the intersection check is the intended ``torch.equal`` (the reference's
    ``assert torch.eq(...)`` at :44 raises for any block larger than 1x1);
  * errors raise instead of opening an IPython shell;
  * tensors given on the CPU are moved to the GPU, results come back on the device of the
    tensor passed to the call (CPU in -> CPU out), so reference call sites run unchanged;
  * ``compute_dtype``: "fp32" (default for fp32 inputs: 1e-4 score parity with the CPU path)
    or "bf16" (default for bf16 inputs: the fused MFMA score+top-k kernel), or "bf16x3" (opt-in: fp32 operands split into
    bf16 hi + lo parts, the fused kernel on the 3K-wide split operands, then an fp32 rescore of its candidates -- the fp32
    route's values without materialising S_hat).
U = pinv(W) (:47,:49): ``pinv_backend="numpy"`` is the reference's own ``numpy.linalg.pinv`` call on the
host (U bit-identical); the default "auto" computes it on the GPU in fp64 (exact pseudo-inverse of the
fp32 block, within 1e-5 of numpy's on the golden cases) and keeps the host call for ill-conditioned
blocks, whose numpy result is an inverse of fp32 round-off.  ``pinv_backend="svd"`` (opt-in) decomposes the block
by Jacobi rotations in fp64 on the GPU and truncates at ``rcond=``: the one route that can leave
that round-off out instead of inverting it.  Every product runs on the GPU.
"""
import logging

import numpy as np
import torch

from . import ops
from .ops import TopK

LOGGER = logging.getLogger(__name__)


def _is_sorted(idx_list):
	"""Strictly increasing (eval/matrix_approx_zeshel.py:53-55)."""
	a = np.asarray(idx_list)
	return bool(np.all(a[:-1] < a[1:]))


def _pinv_host(M, rcond=None):
	"""rcond=None: numpy.linalg.pinv (LAPACK SVD in fp32, rcond=1e-15) on the fp32 values, exactly the reference's call (U bit-identical).
	A given rcond has no counterpart in the reference to stay identical to; that call is the parity reference of the "svd" route, so it runs
	LAPACK in fp64 on the same fp32 values and rounds to fp32 once -- numpy's fp32 SVD is itself ~1e-7 ||X|| away from that."""
	if rcond is None:
		return torch.from_numpy(np.linalg.pinv(M.detach().float().cpu().numpy()))
	return torch.from_numpy(np.linalg.pinv(M.detach().float().cpu().numpy().astype(np.float64), rcond=rcond).astype(np.float32))


COMPUTE_DTYPES = ("fp32", "bf16", "bf16x3")


AUTO_COND_LIMIT = 1e3   # pinv_backend "auto": the device result is taken while cond_2(W) stays below this (numpy's fp32 SVD is then good to ~1e-4)
AUTO_COND_SAFETY = 1.25  # ... times this: the power-iteration estimate of cond_2 is a lower bound, at most this factor short (pinv._spectral_norm_sq)
AUTO_SQUARE_RATIO, AUTO_SQUARE_MIN = 0.9, 32   # "auto": blocks with min(shape) > 0.9 max(shape) (and at least 32 wide) go straight to the host


PINV_BACKENDS = ("auto", "device", "numpy", "device32", "svd")
PINV_RCOND_BACKENDS = ("numpy", "svd")   # the backends that take rcond=: Newton-Schulz ("auto", "device", "device32") cannot truncate


def check_pinv_args(backend, rcond):
	"""The rules of (pinv_backend, rcond) as ValueErrors, before any work: rcond=None is the reference's 1e-15; a given rcond lies in [0, 1)
	and needs a backend that can truncate."""
	if backend not in PINV_BACKENDS:
		raise ValueError(f"pinv_backend = {backend} not supported")
	if rcond is None:
		return None
	if backend not in PINV_RCOND_BACKENDS:
		raise ValueError(f"rcond = {rcond!r} given with pinv_backend = {backend!r}: Newton-Schulz cannot truncate, only pinv_backend {' / '.join(repr(b) for b in PINV_RCOND_BACKENDS)} "
						 "takes rcond")
	return ops._rcond_check(rcond, "pinv")


def _pinv(M, device, backend, rcond=None, info=None):
	"""rcond: the cutoff of the pseudo-inverse relative to the largest singular value (numpy.linalg.pinv's); None = the reference's 1e-15.
	  Only "numpy" and "svd" take one (check_pinv_args).  info: a dict that backend "svd" fills with singular_values (fp64 on the device,
	  descending) and rank, both None where the block went to the host.
	backend "svd": the Jacobi SVD in fp64 on the GPU and the pseudo-inverse truncated at rcond (pinv.pinv_svd), rounded to fp32 once:
	  numpy.linalg.pinv(M, rcond) up to numpy's own fp32 round-off, at any conditioning.  A decomposition that did not converge goes to the
	  host call with the same rcond (logged).  A block outside 1 <= min(shape) <= 2048, max(shape) <= 8192 is a ValueError that names the limit:
	  that excludes the oracle's pinv(C) [n x kc] and pinv(R) [kr x m] at full size -- with A= (cur_oracle) "svd" serves small matrices only.
	backend "numpy": the reference's own call on the host (U bit-identical to the reference); with a given rcond, numpy.linalg.pinv(M, rcond) in fp64
	  on the fp32 values, rounded once (_pinv_host): the parity reference of "svd".
	backend "device": Newton-Schulz in fp64 on the GPU (anncur_amd/pinv.py), rounded to fp32 once: the exact pseudo-inverse of the
	  fp32 matrix; differs from numpy's fp32 LAPACK SVD by numpy's own round-off, ~cond(W) * 6e-8 (measured 1e-6..1e-5 on the
	  golden cases).  A block that is singular to fp32 precision (no convergence within the iteration budget) goes to the host
	  call: what numpy returns there is an inverse of round-off noise that no other algorithm reproduces.
	backend "auto": the device route, kept only where it is as good as pinned -- cond_2(W) = ||W||_2 ||W^+||_2 <= 1e3 (power iteration), where
	  the two agree far inside the 1e-4 score tolerance; an ill-conditioned block (e.g. as many anchor rows as anchor columns:
	  numpy inverts singular values that are fp32 noise, and the reference's numbers are made of that noise) goes to the host call.
	backend "device32": the fp32 iteration of round 1 (fast, ~1e-3)."""
	rcond = check_pinv_args(backend, rcond)
	if backend == "numpy":
		return _pinv_host(M, rcond).to(device)
	if backend == "svd":
		from . import pinv
		if info is not None:
			info.update(singular_values=None, rank=None)
		if min(M.shape) == 0:
			return torch.zeros((M.shape[1], M.shape[0]), dtype=torch.float32, device=device)
		X, res = pinv.pinv_svd(M.to(device), 1e-15 if rcond is None else rcond, return_info=True)
		if res["converged"]:
			if info is not None:
				info.update(singular_values=res["singular_values"], rank=res["rank"])
			return X
		LOGGER.info("pinv svd: %d x %d block not converged after %d sweeps -> host numpy.linalg.pinv", M.shape[0], M.shape[1], res["sweeps"])
		return _pinv_host(M, rcond).to(device)
	if backend in ("device", "auto"):
		from .pinv import pinv_newton_schulz_f64
		if min(M.shape) == 0:
			return torch.zeros((M.shape[1], M.shape[0]), dtype=torch.float32, device=device)
		if backend == "auto" and min(M.shape) >= AUTO_SQUARE_MIN and min(M.shape) > AUTO_SQUARE_RATIO * max(M.shape):
			# (near-)square anchor block (entry A's n_ment_anchors == n_ent_anchors cells): its smallest singular value is ~1/n of the
			# largest, cond_2 far above the limit -- the iteration would burn its budget and end on the host anyway
			LOGGER.info("pinv auto: %d x %d block is (near-)square -> host numpy.linalg.pinv", M.shape[0], M.shape[1])
			return _pinv_host(M).to(device)
		# auto: a block with cond_2 <= 1e3 converges within ~2 log2(cond) + 6 = 26 steps; one that has not by 36 is beyond the limit
		X, info = pinv_newton_schulz_f64(M.to(device), return_info=True, max_iters=36 if backend == "auto" else 64)
		# cond_2 comes from two power iterations (pinv._spectral_norm_sq: 2^POWER_SQUARINGS steps), each a LOWER bound: cond_2 <= true <= AUTO_COND_SAFETY * cond_2 is held
		# by test on clustered, geometric and power-law spectra (tests/test_gpu_pinv_gate.py), hence the safety factor
		if info["converged"] and (backend == "device" or AUTO_COND_SAFETY * info["cond_2"] <= AUTO_COND_LIMIT):
			return X
		LOGGER.info("pinv %s: cond_2 = %.3g after %d iterations (converged: %s) -> host numpy.linalg.pinv", backend, info["cond_2"], info["iterations"], info["converged"])
		return _pinv_host(M).to(device)
	if backend == "device32":
		from .pinv import pinv_newton_schulz
		return pinv_newton_schulz(M.to(device))
	raise ValueError(f"pinv_backend = {backend} not supported")


def _is_full_range(idx, n):
	"""idx is exactly 0..n-1 in order (a permutation or a list with repeats is NOT the identity: the reference's
	latent_rows[row_idxs, :] honours order and duplicates)."""
	if torch.is_tensor(idx):
		idx = idx.detach().cpu().numpy()
	a = np.asarray(idx)
	return a.ndim == 1 and a.shape[0] == n and n > 0 and bool(np.array_equal(a, np.arange(n)))


class CURApprox(object):

	def __init__(self, rows, cols, row_idxs, col_idxs, approx_preference, A=None, compute_dtype=None, device=None, pinv_backend="auto", rcond=None, small_batch=False):
		"""small_batch: compute_dtype "bf16" only -- calls of up to 64 queries take the small-batch route (topk_route names it).
		rcond: the cutoff of U = pinv(W) relative to W's largest singular value, for pinv_backend "svd" and "numpy" (None = the reference's
		1e-15; with any other backend a given rcond is a ValueError).  With "svd" and no A=, singular_values (fp64, descending) and rank (those
		above the cutoff) describe the anchor block W; they are None otherwise, and where the block went to the host."""
		super(CURApprox, self).__init__()
		self.pinv_backend = pinv_backend
		self.rcond = check_pinv_args(pinv_backend, rcond)
		self.singular_values = self.rank = None
		if device is None:
			device = rows.device if (torch.is_tensor(rows) and rows.is_cuda) else torch.device("cuda", torch.cuda.current_device())
		self.device = torch.device(device)
		self._home = rows.device if torch.is_tensor(rows) else torch.device("cpu")

		self.n = cols.shape[0]
		self.m = rows.shape[1]
		self.row_idxs = row_idxs
		self.col_idxs = col_idxs
		# device-resident operands (underscore names); the reference's attribute names C / R / U / latent_rows / latent_cols are
		# properties that hand out tensors on the device the caller's matrices live on (CPU in -> CPU attributes)
		self._C = self._to_dev(cols)  # n x kc
		self._R = self._to_dev(rows)  # kr x m
		self._home_cache = {}
		self.approx_preference = approx_preference
		if compute_dtype is None:
			compute_dtype = "bf16" if self._R.dtype == torch.bfloat16 else "fp32"
		if compute_dtype not in COMPUTE_DTYPES:
			raise ValueError(f"compute_dtype = {compute_dtype} not supported")
		self.compute_dtype = compute_dtype
		self.small_batch = bool(small_batch)

		assert _is_sorted(self.row_idxs), "row_idxs should be sorted"
		assert _is_sorted(self.col_idxs), "col_idxs should be sorted"
		assert len(row_idxs) == self._R.shape[0]
		assert len(col_idxs) == self._C.shape[1]

		intersect_mat = ops.gather_rows(self._C, row_idxs)  # kr x kc
		assert torch.equal(intersect_mat, ops.gather_cols(self._R, col_idxs)), \
			"Invalid rows and cols as their intersection does not match"

		if A is not None:  # oracle U = C^+ A R^+  (:46-47), products left to right on the GPU
			A_dev = self._to_dev(A)
			CpA = ops.gemm(_pinv(self._C, self.device, pinv_backend, self.rcond), A_dev)       # kc x m
			self._U = ops.gemm(CpA, _pinv(self._R, self.device, pinv_backend, self.rcond))     # kc x kr
		else:
			info = {}
			self._U = _pinv(intersect_mat, self.device, pinv_backend, self.rcond, info)       # kc x kr  (:49)
			self.singular_values, self.rank = info.get("singular_values"), info.get("rank")

		self._Et = None   # [m x kc] fp32: latent_cols transposed ("rows" preference)
		self._Etp = None  # bf16 packed copy for the fused kernel
		self._Etp_sorted = self._item_ids = None
		self._split = None  # "bf16x3": the split-bf16 operands of E^T (_SplitOperands)
		self._latent_rows, self._latent_cols = self._build_latent_row_cols(self._C, self._U, self._R, self.approx_preference)

	# ------------------------------------------------------------------ the reference's attributes (matrix_approx_zeshel.py:36-51)
	def _attr(self, name):
		t = getattr(self, "_" + name)
		if t.device == self._home:
			return t
		if name not in self._home_cache:
			self._home_cache[name] = t.to(self._home)
		return self._home_cache[name]

	C = property(lambda self: self._attr("C"))
	R = property(lambda self: self._attr("R"))
	U = property(lambda self: self._attr("U"))
	latent_rows = property(lambda self: self._attr("latent_rows"))
	latent_cols = property(lambda self: self._attr("latent_cols"))

	# ------------------------------------------------------------------ helpers
	def _to_dev(self, t):
		if not torch.is_tensor(t):
			t = torch.as_tensor(np.asarray(t))
		if t.dtype not in (torch.float32, torch.bfloat16):
			t = t.float()
		return t.to(self.device)

	@staticmethod
	def _back(t, like):
		dev = like.device if torch.is_tensor(like) else torch.device("cpu")
		return t if t.device == dev else t.to(dev)

	@staticmethod
	def _is_sorted(idx_list):
		return _is_sorted(idx_list)

	def _build_latent_row_cols(self, C, U, R, approx_preference):
		if approx_preference == "cols":
			latent_rows = ops.gemm(C, U)  # n x kr
			latent_cols = R               # kr x m
		elif approx_preference == "rows":
			latent_rows = C               # n x kc
			# E^T = R^T U^T directly in the item-major layout the score kernels stream ([m x kc], rows contiguous)
			self._Et = ops.gemm(R.t(), U.t())
			latent_cols = self._Et.t()    # kc x m view (= U @ R)
			kp = ops.padded_k(self._Et.shape[1])
			if self.compute_dtype == "bf16" and kp is not None:
				self._Etp = ops.pack_bf16(self._Et, kp, row_multiple=32)               # item order: error terms, dense route
				self._Etp_sorted, self._item_ids = _norm_sorted_pack(self._Et, kp)     # norm order: fused top-k
			if self.compute_dtype == "bf16x3":
				self._split = _SplitOperands.build(self._Et)
		else:
			raise NotImplementedError(f"approx_preference = {approx_preference} not supported")
		return latent_rows, latent_cols

	def _take_rows(self, M, idx):
		return M if _is_full_range(idx, M.shape[0]) else ops.gather_rows(M, idx)

	def _take_cols(self, M, idx):
		if _is_full_range(idx, M.shape[1]):
			return M
		if M.stride(1) == 1 or M.shape[1] == 1:
			return ops.gather_cols(M, idx)
		return ops.gather_rows(M.t(), idx).t()  # column-major view (latent_cols = Et^T): gather item rows of Et

	# ------------------------------------------------------------------ reconstruction (a6)
	def get_rows(self, row_idxs):
		ans = ops.gemm(self._take_rows(self._latent_rows, row_idxs), self._latent_cols)
		return self._back(ans, self._home)

	def get_cols(self, col_idxs):
		ans = ops.gemm(self._latent_rows, self._take_cols(self._latent_cols, col_idxs))
		return self._back(ans, self._home)

	def get(self, row_idxs, col_idxs):
		ans = ops.gemm(self._take_rows(self._latent_rows, row_idxs), self._take_cols(self._latent_cols, col_idxs))
		return self._back(ans, self._home)

	def get_complete_col(self, sparse_cols):
		if self.approx_preference != "cols":
			raise NotImplementedError("This is not designed to give good approx of cols as U matrix is multiplied w/ R matrix. Build index w/ approx_preference = cols instead.")
		return self._back(ops.gemm(self._latent_rows, self._to_dev(sparse_cols)), sparse_cols)

	def topk_in_col(self, sparse_cols, k):
		if self.approx_preference != "cols":
			raise NotImplementedError("This is not designed to give good approx of cols as U matrix is multiplied w/ R matrix. Build index w/ approx_preference = cols instead.")
		dense = ops.gemm(self._latent_rows, self._to_dev(sparse_cols))
		v, i = ops.rowwise_topk(dense, k)
		return TopK(self._back(v, sparse_cols), self._back(i.long(), sparse_cols))

	def get_complete_row(self, sparse_rows):
		if self.approx_preference != "rows":
			raise NotImplementedError("This is not designed to give good approx of rows as C and U matrix are multiplied together. Build index w/ approx_preference = rows instead.")
		return self._back(ops.gemm(self._to_dev(sparse_rows), self._latent_cols), sparse_rows)

	# ------------------------------------------------------------------ retrieval (a6 + a7)
	def topk_in_row_device(self, sparse_rows, k, exclude=None):
		"""(values f32 [Q,k], indices int32 [Q,k]) on the GPU; S_hat is never materialised on the bf16 route.
		exclude: items left out of the result (ops.exclusion: one list for all queries, one per query, or a -1 padded [Q x w] array; rows
		with fewer than k items left end in (-inf, -1)).  The route retrieves k + the longest list and one filter launch trims it."""
		if self.approx_preference != "rows":
			raise NotImplementedError("This is not designed to give good approx of rows as C and U matrix are multiplied together. Build index w/ approx_preference = rows instead.")
		X = self._to_dev(sparse_rows)
		Q = X.shape[0]
		excl, kc = _exclusion_arg(exclude, Q, self.m, k, self.device)
		if self._split is not None and self._split.takes(Q, self.m, k, excl):
			return self._split.topk(X, self._Et, k, excl)
		if _few_takes(self, Q, kc):
			return _filtered(ops.score_topk_few(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp, self.m, kc), excl, k)
		if self._Etp is not None and ops.fused_supported(Q, self.m, self._Etp.shape[1], kc):
			return _filtered(ops.score_topk_fused(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp_sorted, self.m, kc, leading_sample=True, item_ids=self._item_ids), excl, k)
		Et = self._Et if self.compute_dtype != "bf16" else (self._Etp[:self.m, :X.shape[1]] if self._Etp is not None else self._Et)
		if self.compute_dtype == "bf16" and X.dtype != torch.bfloat16:
			X = ops.convert(X, torch.bfloat16)
		return _filtered(ops.score_topk_dense(X, Et, kc), excl, k)

	def topk_route(self, Q, k, exclude=None):
		"""The route topk_in_row takes for Q queries and k results: "bf16x3", "bf16-few", "bf16" or "dense" (_route_name)."""
		excl, _ = _exclusion_arg(exclude, Q, self.m, k, self.device)
		return _route_name(self, Q, k, excl)

	def topk_in_row(self, sparse_rows, k, exclude=None):
		v, i = self.topk_in_row_device(sparse_rows, k, exclude=exclude)
		return TopK(self._back(v, sparse_rows), self._back(i.long(), sparse_rows))

	def rank_route(self, t):
		"""The route rank_in_row takes for t targets per query: "bf16" (fused, S_hat never written) or "dense"."""
		return _rank_route_name(self, t)

	def rank_in_row(self, sparse_rows, ids, return_scores=False):
		"""The inverse of topk_in_row: rank[q, j] = the position of item ids[q, j] in row q of the approximation sorted by score descending,
		ties to the smaller id (ops.rank_in_rows states the contract: -1 for a hole or a NaN score, at most ops.RANK_MAX_T targets per query).
		int32 [Q x t], on the device of sparse_rows; with return_scores (rank, score).  compute_dtype "bf16" with Kp <= 512 never writes S_hat."""
		if self.approx_preference != "rows":
			raise NotImplementedError("This is not designed to give good approx of rows as C and U matrix are multiplied together. Build index w/ approx_preference = rows instead.")
		res = _route_rank(self, self._to_dev(sparse_rows), ids, return_scores)
		return tuple(self._back(r, sparse_rows) for r in res) if return_scores else self._back(res, sparse_rows)

	def eval_rows(self, sparse_rows, exact_rows, k):
		"""One grid cell of entry point A for these query rows (crossenc.py:84,106,146-147): (approximate top-k of S_hat, per-row
		sum (S_hat - A)^2, per-row sum A^2).  On the bf16 route with Kp <= 256 and a bf16 exact matrix this is ONE sweep
		(ops.eval_fused: the kernel that streams the exact tile beside the MFMA chain also filters its accumulator for candidates);
		otherwise the two calls topk_in_row_device + approx_error_rows."""
		if self.approx_preference != "rows":
			raise NotImplementedError("This is not designed to give good approx of rows as C and U matrix are multiplied together. Build index w/ approx_preference = rows instead.")
		X, A = self._to_dev(sparse_rows), self._to_dev(exact_rows)
		if (self.compute_dtype == "bf16" and self._Etp is not None and ops.eval_fused_ok(self._Etp.shape[1], A, X.shape[0], self.m, k)):
			return ops.eval_fused(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp, A, self.m, k, hint=self._Etp_sorted)
		approx = self.topk_in_row_device(sparse_rows, k)
		err, nrm = self.approx_error_rows(sparse_rows, exact_rows)
		return approx, err, nrm

	def approx_error_rows(self, sparse_rows, exact_rows):
		"""Per-row sum (S_hat - A)^2 and sum A^2 (a11) without materialising S_hat.  On the bf16 route S_hat is the one the retrieval
		ranks (bf16 item embeddings), computed on the sweep's MFMA loop."""
		X, A = self._to_dev(sparse_rows), self._to_dev(exact_rows)
		if self._split is not None and ops.approx_error_packed_ok(self._split.kp, A):
			return self._split.approx_error(X, self._Et, A)
		if self.compute_dtype == "bf16" and self._Etp is not None and ops.approx_error_packed_ok(self._Etp.shape[1], A):
			return ops.approx_error_packed(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp, A, self.m)
		return ops.approx_error(X, self._Et, A)


def _exclusion_arg(exclude, Q, m, k, device):
	"""(Exclusion or None, candidates per query the route retrieves) for a top-k's `exclude=` argument.  Nothing to exclude -- None, empty
	lists -- gives (None, k): the call then runs exactly as it does without the argument."""
	if exclude is None:
		return None, k
	excl = ops.exclusion(exclude, Q, m, device)
	if excl.e_max == 0:
		return None, k
	return excl, ops.filtered_k(k, excl.e_max, m)


def _filtered(res, excl, k):
	return res if excl is None else ops.filter_topk(res.values, res.indices, excl, k)


def _norm_sorted_pack(Et, kp):
	"""(packed bf16 E^T with its rows ordered by descending norm, int32 map row -> item id): the index builder's hint for the fused
	top-k (anncur_score_topk_ex): items with a large ||E_i|| are the likeliest high scorers, so a threshold sampled from the leading
	rows -- and a sweep that meets them first -- lets far fewer elements through (-40 % on the synthetic protocol, whose norms vary
	by only 7 %).  The result is unchanged: the exact top-k of S_hat, reported with the original item ids."""
	order = ops.descending_norm_order(Et if Et.dtype == torch.float32 else ops.convert(Et, torch.float32))   # 256 norm buckets, stable inside a bucket
	return ops.pack_bf16(ops.gather_rows(Et, order), kp, row_multiple=32), order


class _SplitOperands(object):
	"""The item side of the "bf16x3" route: E^T [m x K] fp32 split into bf16 hi + lo parts and packed as [hi | lo | hi]
	rows of width Kp = split_kp(K), once in the descending-norm order of _norm_sorted_pack (the fused top-k, with the map back to item
	ids) and -- lazily, only when the error sums ask for it -- once in item order.  kp is None where 3 K is too wide for the fused
	kernels: every call then takes the fp32 route."""

	def __init__(self, kp, sorted_pack, item_ids):
		self.kp, self.sorted, self.item_ids = kp, sorted_pack, item_ids
		self._item_order = None

	@classmethod
	def build(cls, Et):
		kp = ops.split_kp(Et.shape[1])
		if kp is None:
			return cls(None, None, None)
		order = ops.descending_norm_order(Et if Et.dtype == torch.float32 else ops.convert(Et, torch.float32))
		return cls(kp, ops.pack_split_bf16(ops.gather_rows(Et, order), 1, kp, row_multiple=32), order)

	def takes(self, Q, m, k, excl=None):
		e = excl.e_max if excl is not None else 0
		return self.kp is not None and k + e <= min(m, ops._lib.MAX_TOPK) and ops.fused_supported(Q, m, self.kp, ops.split_candidates(m, k, n_excl=e))

	def topk(self, X, Et, k, excl=None):
		return ops.score_topk_split(X, Et, self.sorted, Et.shape[0], k, item_ids=self.item_ids, leading_sample=True, exclude=excl)

	def approx_error(self, X, Et, A):
		"""a11 on the split operands (the sweep's bf16 MFMA loop, Kp <= 512): S_hat within (2^-16 + 3K 2^-23) |X|.|E|^T of the fp32 one."""
		if self._item_order is None:
			self._item_order = ops.pack_split_bf16(Et, 1, self.kp, row_multiple=32)
		return ops.approx_error_packed(ops.pack_split_bf16(X, 0, self.kp), self._item_order, A, Et.shape[0])


def _few_takes(op, Q, kc):
	"""The small-batch route: only where the index was built with small_batch=True on the "bf16" operands, for up to 64
	queries; "fp32" and "bf16x3" indices ignore the flag."""
	return (getattr(op, "small_batch", False) and op.compute_dtype == "bf16" and op._Etp is not None and kc <= min(op.m, ops._lib.MAX_TOPK)
			and ops.score_topk_few_ok(Q, op.m, op._Etp.shape[1], kc))


def _route_name(op, Q, k, excl=None):
	"""Which of the top-k routes `op` (a CURRowIndex, a CURApprox or an _ItemOperand) takes for Q queries and k results: "bf16x3" (split
	operands + fp32 rescore), "bf16-few" (small_batch=True and Q <= 64: the streamed score + group-sparse select), "bf16" (fused sweep) or
	"dense" (fp32 / bf16 GEMM + exact scan)."""
	kc = k + (excl.e_max if excl is not None else 0)
	if op._split is not None and op._split.takes(Q, op.m, k, excl):
		return "bf16x3"
	if _few_takes(op, Q, kc):
		return "bf16-few"
	if op._Etp is not None and kc <= min(op.m, ops._lib.MAX_TOPK) and ops.fused_supported(Q, op.m, op._Etp.shape[1], kc):
		return "bf16"
	return "dense"


def _route_topk(op, X, k, exclude=None):
	"""Top-k of X . Et^T over the item operand of `op` (CURRowIndex: E^T; _ItemOperand: any item-major matrix), routed by op.compute_dtype
	and by what the fused kernels take; exclude as for CURApprox.topk_in_row_device."""
	Q = X.shape[0]
	excl, kc = _exclusion_arg(exclude, Q, op.m, k, X.device)
	if op._split is not None and op._split.takes(Q, op.m, k, excl):
		return op._split.topk(X, op._Et, k, excl)
	if _few_takes(op, Q, kc):
		return _filtered(ops.score_topk_few(ops.pack_bf16(X, op._Etp.shape[1]), op._Etp, op.m, kc), excl, k)
	if op._Etp is not None and ops.fused_supported(Q, op.m, op._Etp.shape[1], kc):
		return _filtered(ops.score_topk_fused(ops.pack_bf16(X, op._Etp.shape[1]), op._Etp_sorted, op.m, kc, leading_sample=True, item_ids=op._item_ids), excl, k)
	Et = op._Et if op.compute_dtype != "bf16" or op._Etp is None else op._Etp[:op.m, :X.shape[1]]
	if op.compute_dtype == "bf16" and X.dtype != torch.bfloat16:
		X = ops.convert(X, torch.bfloat16)
	return _filtered(ops.score_topk_dense(X, Et, kc), excl, k)


def _rank_ids_arg(ids, device):
	"""Target ids as the index classes take them -- a list, a NumPy array or a tensor, int32 or int64, e.g. the indices of a top-k or a slice of
	them -- as a contiguous int32 tensor on `device`.  A value outside int32 cannot be an item id: ValueError, before the narrowing hides it."""
	ids = ids if torch.is_tensor(ids) else torch.as_tensor(np.asarray(ids))
	if ids.dtype not in (torch.int32, torch.int64):
		raise TypeError(f"rank: ids must be int32 or int64 (got {ids.dtype})")
	if ids.dim() != 2:
		raise ValueError(f"rank: ids must be [Q x t] (got {tuple(ids.shape)})")
	if ids.dtype == torch.int64:
		if ids.numel():
			lo, hi = (int(v) for v in torch.aminmax(ids))
			if lo < -1 or hi >= 1 << 31:
				raise ValueError(f"rank: id {lo if lo < -1 else hi} is no item id")
		ids = ids.to(torch.int32)
	return ids.to(device).contiguous()


def _rank_route_name(op, t):
	"""Which of the two rank routes `op` takes for t targets per query: "bf16" (ops.score_rank on the item-order packed operand, S_hat never
	written) or "dense" (ops.rank_dense on the fp32 item operand -- "fp32", "bf16x3", Kp > 512 and whatever the fused route refuses: the
	values the "bf16x3" top-k returns)."""
	if op.compute_dtype == "bf16" and op._Etp is not None and ops.score_rank_ok(op._Etp.shape[1], op.m, t):
		return "bf16"
	return "dense"


def _route_rank(op, X, ids, return_scores=False):
	"""Ranks of the items ids [Q x t] under X . Et^T over the item operand of `op` (ops.rank_in_rows states the contract), beside _route_topk."""
	ids = _rank_ids_arg(ids, X.device)
	if _rank_route_name(op, ids.shape[1]) == "bf16":
		return ops.score_rank(ops.pack_bf16(X, op._Etp.shape[1]), op._Etp, op.m, ids, return_scores)
	if X.dtype != torch.float32:
		X = ops.convert(X, torch.float32)
	return ops.rank_dense(X, op._Et, ids, return_scores=return_scores)


class _RankOperand(object):
	"""An item-major fp32 matrix Et [m x K] prepared for _route_rank: "bf16" packs it in ITEM order where the fused route takes the width."""

	def __init__(self, Et, compute_dtype):
		self._Et, self.m, self.compute_dtype = Et, Et.shape[0], compute_dtype
		kp = ops.padded_k(Et.shape[1])
		self._Etp = ops.pack_bf16(Et, kp, row_multiple=32) if compute_dtype == "bf16" and kp is not None and kp <= 512 else None


SAMPLE_ROUTE = "sample-dense"   # the one route of _route_sample, as the adaptive search's trace names it


def _route_sample(op, X, k, temperature=1.0, seed=0, stream=0, row_keys=None, exclude=None):
	"""k items per query drawn without replacement with probability proportional to softmax(X . Et^T / temperature) over the item operand
	of `op` (ops.sample_topk_dense: the noise contract, row_keys and exclude are ops.sample_topk's).  ONE route, whatever op.compute_dtype is:
	the fp32 item operand, a dense fp32 GEMM per row chunk and the sampler on it.  Sampling has no fused route -- the noise differs per
	(query, item) pair, so it cannot ride in the MFMA operands, and a sample inside an over-fetched head is not a sample of the softmax
	(DESIGN 4.4e)."""
	if X.dtype != torch.float32:
		X = ops.convert(X, torch.float32)
	return ops.sample_topk_dense(X, op._Et, k, temperature, seed, stream, row_keys, exclude)


class _ItemOperand(object):
	"""An item-major fp32 matrix Et [m x K] prepared for _route_topk the way CURRowIndex prepares E^T: "bf16" packs it (item order and
	descending-norm order with the id map), "bf16x3" builds the split operands, "fp32" keeps it as it is."""

	def __init__(self, Et, compute_dtype, small_batch=False):
		self._Et, self.m, self.compute_dtype, self.small_batch = Et, Et.shape[0], compute_dtype, bool(small_batch)
		kp = ops.padded_k(Et.shape[1])
		self._Etp = self._Etp_sorted = self._item_ids = None
		if compute_dtype == "bf16" and kp is not None:
			self._Etp = ops.pack_bf16(Et, kp, row_multiple=32)
			self._Etp_sorted, self._item_ids = _norm_sorted_pack(Et, kp)
		self._split = _SplitOperands.build(Et) if compute_dtype == "bf16x3" else None

	def topk(self, X, k, exclude=None):
		return _route_topk(self, X, k, exclude)

	def route(self, Q, k, exclude=None):
		excl, _ = _exclusion_arg(exclude, Q, self.m, k, self._Et.device)
		return _route_name(self, Q, k, excl)

	def sample(self, X, k, temperature=1.0, seed=0, stream=0, row_keys=None, exclude=None):
		return _route_sample(self, X, k, temperature, seed, stream, row_keys, exclude)


ANCHOR_SELECTIONS = ("random", "pivoted")


class AnchorSelection(object):
	"""Anchor items in SELECTION order (select_anchor_items).  order: np.int64 [n_sel]; gains: np.float64 [n_sel], the squared residual norm
	each item had when the pivoted selection took it (None for "random").  The pivoted selection is nested: sorted(n) is the anchor set of n
	items for every n <= n_sel, in the sorted form CURApprox / CURRowIndex take as col_idxs."""

	def __init__(self, order, gains=None):
		self.order = np.asarray(order, dtype=np.int64).reshape(-1)
		self.gains = None if gains is None else np.asarray(gains, dtype=np.float64).reshape(-1)

	@property
	def n_sel(self):
		return int(self.order.shape[0])

	def sorted(self, n=None):
		n = self.n_sel if n is None else n
		if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
			raise ValueError(f"AnchorSelection.sorted: n must be an integer >= 0 (got {n!r})")
		if n > self.n_sel:
			raise ValueError(f"AnchorSelection.sorted: n = {n} anchor items asked of a selection of n_sel = {self.n_sel}")
		return sorted(int(i) for i in self.order[:n])


def select_anchor_items(rows, n, method="pivoted", rng=None):
	"""The index' choice of its n anchor items from the anchor rows `rows` [kq x m] -> AnchorSelection.
	"pivoted": column-pivoted QR of rows on the device (ops.select_pivoted): deterministic, nested, and it stops at the numerical
	  rank, so n_sel may be below n.  rows on the CPU are moved to the GPU.
	"random": sorted(rng.choice(m, n, replace=False)), the reference's selection (..._splits.py:295) from the caller's generator `rng`."""
	if method not in ANCHOR_SELECTIONS:
		raise ValueError(f"select_anchor_items: method = {method!r}, need one of {ANCHOR_SELECTIONS}")
	m = rows.shape[1]
	if method == "random":
		if rng is None:
			raise ValueError("select_anchor_items: method 'random' needs rng= (a numpy Generator)")
		return AnchorSelection(sorted(rng.choice(m, size=n, replace=False)))
	if rng is not None:
		raise ValueError("select_anchor_items: method 'pivoted' is deterministic and takes no rng")
	if torch.is_tensor(rows) and not rows.is_cuda:
		rows = rows.cuda()
	ids, gains, n_sel = ops.select_pivoted(rows, n)
	return AnchorSelection(ids[:n_sel].cpu().numpy(), gains[:n_sel].cpu().numpy())


class CURRowIndex(object):
	"""The "rows"-preference index alone: built from the anchor rows R [kr x m] and the anchor columns' ids, without the
	(n x kc) matrix of every query's anchor scores.  This is what a rank of a row-sharded evaluation holds: R assembled by one
	all-gather, U = pinv(R[:, col_idxs]) and E = U.R replicated, its own queries' anchor scores gathered locally.
	Same arithmetic as CURApprox(rows=R, cols=A[:, col_idxs], ...) (eval/matrix_approx_zeshel.py:42-65)."""

	def __init__(self, rows, col_idxs, compute_dtype=None, pinv_backend="auto", rcond=None, small_batch=False):
		"""small_batch: compute_dtype "bf16" only -- calls of up to 64 queries (topk, and the adaptive search's rounds) take the small-batch
		route (topk_route names the route of a call).  rcond, and the attributes singular_values / rank that pinv_backend "svd" fills: as for CURApprox."""
		self.rcond = check_pinv_args(pinv_backend, rcond)
		self.R = rows
		self.m = rows.shape[1]
		self.col_idxs = col_idxs
		if compute_dtype is None:
			compute_dtype = "bf16" if rows.dtype == torch.bfloat16 else "fp32"
		if compute_dtype not in COMPUTE_DTYPES:
			raise ValueError(f"compute_dtype = {compute_dtype} not supported")
		self.compute_dtype = compute_dtype
		self.small_batch = bool(small_batch)
		W = ops.gather_cols(rows, col_idxs)                      # kr x kc
		info = {}
		self.U = _pinv(W, rows.device, pinv_backend, self.rcond, info)   # kc x kr
		self.singular_values, self.rank = info.get("singular_values"), info.get("rank")
		self._Et = ops.gemm(rows.t(), self.U.t())                # m x kc
		kp = ops.padded_k(self._Et.shape[1])
		self._Etp = self._Etp_sorted = self._item_ids = None
		if compute_dtype == "bf16" and kp is not None:
			self._Etp = ops.pack_bf16(self._Et, kp, row_multiple=32)
			self._Etp_sorted, self._item_ids = _norm_sorted_pack(self._Et, kp)
		self._split = _SplitOperands.build(self._Et) if compute_dtype == "bf16x3" else None
		self._adaptive = None   # adaptive_operand(), built at the first adaptive search

	def topk(self, X, k, exclude=None):
		"""X [q x kc]: the queries' exact scores against the anchor items -> (values f32, indices int32) on the GPU.
		exclude: items left out of the result, as for CURApprox.topk_in_row_device (e.g. ops.exclusion(self.col_idxs, ...), built once:
		the anchor items, whose exact scores the caller holds already)."""
		return _route_topk(self, X, k, exclude)

	def topk_route(self, Q, k, exclude=None):
		"""The route topk() takes for Q queries and k results: "bf16x3", "bf16-few", "bf16" or "dense" (_route_name)."""
		excl, _ = _exclusion_arg(exclude, Q, self.m, k, self._Et.device)
		return _route_name(self, Q, k, excl)

	def rank_route(self, t):
		"""The route rank_of() takes for t targets per query: "bf16" (fused, S_hat never written) or "dense"."""
		return _rank_route_name(self, t)

	def rank_of(self, X, ids, return_scores=False):
		"""The inverse of topk: X [q x kc], ids [q x t] (int32 / int64, -1 = hole) -> rank int32 [q x t] on the GPU, the position of each item in
		its query's approximate ranking (score descending, ties to the smaller id; ops.rank_in_rows states the contract); with return_scores
		(rank, score).  rank_of(X, exact_top_k_ids) is the whole recall curve at once: retrieval.overlap_from_ranks / rank_curve.
		(Not `rank`: that name is the attribute pinv_backend "svd" fills with the anchor block's numerical rank.)"""
		return _route_rank(self, X, ids, return_scores)

	def sample(self, X, k, temperature=1.0, seed=0, stream=0, row_keys=None, exclude=None):
		"""X [q x kc] -> TopK(perturbed keys f32, indices int32) on the GPU: k items per query drawn without replacement with probability
		proportional to softmax(S_hat / temperature), S_hat = X . E (ops.sample_topk: Gumbel top-k, reproducible from seed, stream and
		row_keys; exclude as for topk).  Always on the fp32 item operand, whatever compute_dtype is: sampling has no fused route
		(_route_sample says why)."""
		return _route_sample(self, X, k, temperature, seed, stream, row_keys, exclude)

	def adaptive_operand(self):
		"""The operand of the adaptive search's retrieval, built at the first call: the anchor rows themselves as ITEM
		embeddings -- Rt fp32 [m x kq], row i = item i's scores under the kq anchor queries -- behind the same three routes as E^T."""
		if self._adaptive is None:
			R = self.R if self.R.dtype == torch.float32 else ops.convert(self.R, torch.float32)
			self._adaptive = _ItemOperand(R.t().contiguous(), self.compute_dtype, self.small_batch)   # (a copy, no arithmetic)
		return self._adaptive

	def eval_topk(self, X, exact_rows, k, k_retvr):
		"""(exact top-k of exact_rows, approximate top-k_retvr of X) -- the two rankings of the reference's per-query loop
		(crossenc.py:97-106).  The exact scan (HBM-bound) runs on a second stream beside the retrieval (MFMA-bound) and is joined before
		the call returns; the retrieval is self.topk(), i.e. chunked over the queries above the workspace limit.  (ops.eval_topk's
		row-chunk co-scheduling is kept as an op but lost to this placement at every size measured: DESIGN 4.1 / bench.py --scan-mode.)"""
		dev = exact_rows.device
		Q = exact_rows.shape[0]
		ev = torch.empty((Q, k), dtype=torch.float32, device=dev)
		ei = torch.empty((Q, k), dtype=torch.int32, device=dev)   # (allocated on the launch stream: no record_stream needed after the join)
		main, side = torch.cuda.current_stream(dev), ops.aux_stream(dev)
		side.wait_stream(main)
		with torch.cuda.stream(side):
			exact = ops.rowwise_topk(exact_rows, k, out=(ev, ei))
		approx = self.topk(X, k_retvr)
		main.wait_stream(side)
		return exact, approx

	def eval_cell(self, X, exact_rows, k, k_retvr):
		"""Everything one grid cell of entry point A needs for these query rows (crossenc.py:97-106,146-147): (exact top-k of exact_rows,
		approximate top-k_retvr, per-row sum (S_hat - A)^2, per-row sum A^2).  The HBM-bound exact scan runs on a second stream beside
		ONE sweep that yields the candidates and the error sums (ops.eval_fused) where the fused route takes the cell; otherwise beside
		the retrieval, followed by the error kernel."""
		dev = exact_rows.device
		Q = exact_rows.shape[0]
		ev = torch.empty((Q, k), dtype=torch.float32, device=dev)
		ei = torch.empty((Q, k), dtype=torch.int32, device=dev)
		main, side = torch.cuda.current_stream(dev), ops.aux_stream(dev)
		side.wait_stream(main)
		with torch.cuda.stream(side):
			exact = ops.rowwise_topk(exact_rows, k, out=(ev, ei))
		if self.compute_dtype == "bf16" and self._Etp is not None and ops.eval_fused_ok(self._Etp.shape[1], exact_rows, Q, self.m, k_retvr):
			approx, err, nrm = ops.eval_fused(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp, exact_rows, self.m, k_retvr, hint=self._Etp_sorted)
		else:
			approx = self.topk(X, k_retvr)
			err, nrm = self.approx_error_rows(X, exact_rows)
		main.wait_stream(side)
		return exact, approx, err, nrm

	def approx_error_rows(self, X, exact_rows):
		if self._split is not None and ops.approx_error_packed_ok(self._split.kp, exact_rows):
			return self._split.approx_error(X, self._Et, exact_rows)
		if self.compute_dtype == "bf16" and self._Etp is not None and ops.approx_error_packed_ok(self._Etp.shape[1], exact_rows):
			return ops.approx_error_packed(ops.pack_bf16(X, self._Etp.shape[1]), self._Etp, exact_rows, self.m)
		return ops.approx_error(X, self._Et, exact_rows)
