"""Tensor-level wrappers over the C ABI.  torch is used only for device memory and the
current HIP stream; all arithmetic happens in libanncur_hip.so.

Every function takes CUDA(HIP) tensors and raises on CPU tensors: there is no CPU path.
"""
from collections import namedtuple
import ctypes
import functools
import itertools

import numpy as np
import torch

from . import _lib
from ._lib import F32, BF16, check

TopK = namedtuple("TopK", ["values", "indices"])

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def _dt(t):
	try:
		return _DT[t.dtype]
	except KeyError:
		raise TypeError(f"unsupported dtype {t.dtype}: anncur_amd kernels take float32 or bfloat16") from None


def _dev(*ts):
	for t in ts:
		if not (torch.is_tensor(t) and t.is_cuda):
			raise _lib.AnncurHipError("anncur_amd ops need tensors on the GPU (cuda/HIP device); there is no CPU fallback")


def _stream():
	return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(fn):
	"""Run the op with its tensors' GPU as the current device: the launch stream (_stream()), the library's per-device caches
	(dynamic-LDS attribute, CU count) and torch's own allocations / fills inside the op then all belong to the device that holds
	the operands, whatever the process' current device is (CURApprox(device=...), --device cuda:N).  Operands on two different
	GPUs are an error."""
	@functools.wraps(fn)
	def wrapped(*args, **kwargs):
		dev = None
		for a in itertools.chain(args, kwargs.values()):
			if torch.is_tensor(a) and a.is_cuda:
				if dev is None:
					dev = a.device
				elif a.device != dev:
					raise _lib.AnncurHipError(f"{fn.__name__}: operands live on different devices ({dev} and {a.device})")
		if dev is None or dev.index == torch.cuda.current_device():
			return fn(*args, **kwargs)
		with torch.cuda.device(dev):
			return fn(*args, **kwargs)
	return wrapped


def _p(t):
	return ctypes.c_void_p(t.data_ptr())


def _rowmajor(t):
	"""2-D tensor with unit column stride (rows may be padded)."""
	if t.dim() != 2:
		raise ValueError("expected a 2-D tensor")
	if t.shape[1] > 1 and t.stride(1) != 1:
		t = t.contiguous()
	if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
		t = t.contiguous()
	return t


def _ld(t):
	return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _wide_queries(Xp):
	"""The fused path's query operand for the wide kernel (Kp > 512): its query rows are addressed with 32-bit offsets inside a 256-row
	block (255 rows x pitch x 2 bytes, csrc/score_fused.hip wide_query_offsets_fit), which anncur_score_topk refuses beyond; a longer pitch
	(a column slice of a very wide matrix) is passed as a compact copy [Q x Kp]."""
	if Xp.shape[1] > 512 and 255 * _ld(Xp) * 2 + 64 >= 1 << 32:
		return Xp.contiguous()
	return Xp


def as_index(idx, device, n=None):
	"""Python list / numpy / tensor of indices -> int32 device tensor.  With `n` (the size of the indexed dimension) host-side
	indices get torch's indexing semantics: negative values wrap, anything outside [-n, n) raises IndexError (the kernels' own
	clamp -- zeros for a bad index -- is only a safety net).  Indices that already live on the GPU are taken as they are: checking
	them would cost a device synchronisation."""
	if torch.is_tensor(idx) and idx.is_cuda:
		return idx.to(device=device, dtype=torch.int32).contiguous()
	a = idx.detach().numpy() if torch.is_tensor(idx) else np.asarray(idx)
	a = a.astype(np.int64, copy=False).reshape(-1)
	if n is not None and a.size:
		lo, hi = int(a.min()), int(a.max())
		if lo < -n or hi >= n:
			raise IndexError(f"index {lo if lo < -n else hi} is out of bounds for dimension with size {n}")
		if lo < 0:
			a = np.where(a < 0, a + n, a)
	return torch.as_tensor(a, dtype=torch.int32).to(device)


# ------------------------------------------------------------------ a2
@_on_device
def gather_cols(A, col_idx, out_dtype=None):
	"""A[:, col_idx]  (reference: eval/run_retrieval_eval_wrt_exact_crossenc.py:74)."""
	_dev(A)
	A = _rowmajor(A)
	idx = as_index(col_idx, A.device, A.shape[1])
	out = torch.empty((A.shape[0], idx.numel()), dtype=out_dtype or A.dtype, device=A.device)
	check(_lib.load().anncur_gather_cols(_p(A), _dt(A), A.shape[0], A.shape[1], _ld(A), _p(idx), idx.numel(), _p(out), _dt(out),
										 max(idx.numel(), 1), _stream()), "gather_cols")
	return out


@_on_device
def gather_rows(A, row_idx, out_dtype=None):
	"""A[row_idx, :]  (reference: eval/run_retrieval_eval_wrt_exact_crossenc.py:73)."""
	_dev(A)
	A = _rowmajor(A)
	idx = as_index(row_idx, A.device, A.shape[0])
	out = torch.empty((idx.numel(), A.shape[1]), dtype=out_dtype or A.dtype, device=A.device)
	n = idx.numel()
	for s in range(0, n, 65535):  # grid.y limit
		e = min(n, s + 65535)
		check(_lib.load().anncur_gather_rows(_p(A), _dt(A), A.shape[0], A.shape[1], _ld(A), _p(idx[s:e]), e - s, _p(out[s:e]), _dt(out),
											 max(A.shape[1], 1), _stream()), "gather_rows")
	return out


@_on_device
def convert(src, dtype):
	_dev(src)
	src = _rowmajor(src)
	out = torch.empty(src.shape, dtype=dtype, device=src.device)
	check(_lib.load().anncur_convert(_p(src), _dt(src), _ld(src), _p(out), _dt(out), max(out.shape[1], 1), src.shape[0], src.shape[1],
									 _stream()), "convert")
	return out


# ------------------------------------------------------------------ a4/a5/a6
@_on_device
def gemm(A, B, out=None, out_dtype=torch.float32, alpha=1.0, beta=0.0, cin=None):
	"""C = alpha * A @ B (+ beta * cin) for 2-D tensors with ARBITRARY strides (transposed views cost nothing);
	fp32 products and sums (exact fmaf chains on the matrix cores).  cin: fp32 [M, N], may be `out` itself."""
	_dev(A, B)
	M, K = A.shape
	K2, N = B.shape
	if K != K2:
		raise ValueError(f"gemm: inner dimensions differ ({K} vs {K2})")
	if out is None:
		out = torch.empty((M, N), dtype=out_dtype, device=A.device)
	elif tuple(out.shape) != (M, N):
		raise ValueError("gemm: out has the wrong shape")
	lib = _lib.load()
	for m0 in range(0, max(M, 1), 65535 * 128):  # grid.y limit of one launch
		m1 = min(M, m0 + 65535 * 128)
		a, c = A[m0:m1], out[m0:m1]
		if cin is None and alpha == 1.0:
			check(lib.anncur_gemm(_p(a), _dt(A), A.stride(0), A.stride(1), _p(B), _dt(B), B.stride(0), B.stride(1), _p(c), _dt(out),
								  out.stride(0), out.stride(1), m1 - m0, N, K, _stream()), "gemm")
		else:
			if cin is not None and (cin.dtype != torch.float32 or tuple(cin.shape) != (M, N)):
				raise ValueError("gemm: cin must be fp32 [M, N]")
			ci = cin[m0:m1] if cin is not None else None
			check(lib.anncur_gemm_ex(_p(a), _dt(A), A.stride(0), A.stride(1), _p(B), _dt(B), B.stride(0), B.stride(1), _p(c), _dt(out),
									 out.stride(0), out.stride(1), m1 - m0, N, K, float(alpha), float(beta),
									 _p(ci) if ci is not None else None, ci.stride(0) if ci is not None else 0, ci.stride(1) if ci is not None else 0,
									 _stream()), "gemm_ex")
	return out


@_on_device
def sumsq(A, out=None, ordered=True):
	"""Frobenius norm squared of an fp32 matrix -> 1-element device tensor (no host sync).  ordered (default): the sum is taken in an order
	that depends on the shape alone, so equal inputs give equal bits (anncur_sumsq_ordered); False: partial sums meet by atomic adds in
	the order the waves finish (anncur_sumsq), and the last bits differ from call to call."""
	_dev(A)
	A = _rowmajor(A)
	if A.dtype != torch.float32:
		raise TypeError("sumsq takes fp32")
	out = torch.empty(1, dtype=torch.float32, device=A.device) if out is None else out
	if ordered:
		partials = torch.empty(_lib.SUMSQ_PARTIALS, dtype=torch.float32, device=A.device)
		check(_lib.load().anncur_sumsq_ordered(_p(A), A.shape[0], A.shape[1], _ld(A), _p(partials), _p(out), _stream()), "sumsq_ordered")
	else:
		check(_lib.load().anncur_sumsq(_p(A), A.shape[0], A.shape[1], _ld(A), _p(out), _stream()), "sumsq")
	return out


@_on_device
def scale_copy(src, dst, alpha=1.0, divide_by=None):
	"""dst[i, j] = alpha / divide_by[0] * src[i, j] for fp32 2-D tensors with arbitrary strides (e.g. a scaled transpose)."""
	_dev(src, dst)
	if src.dtype != torch.float32 or dst.dtype != torch.float32 or tuple(src.shape) != tuple(dst.shape):
		raise ValueError("scale_copy: fp32 tensors of equal shape")
	check(_lib.load().anncur_scale_copy(_p(src), src.stride(0), src.stride(1), _p(dst), dst.stride(0), dst.stride(1), src.shape[0], src.shape[1],
										float(alpha), _p(divide_by) if divide_by is not None else None, _stream()), "scale_copy")
	return dst


# ------------------------------------------------------------------ fp64 helpers of the on-device pseudo-inverse
@_on_device
def gemm_f64(A, B, out=None, alpha=1.0, beta=0.0, cin=None):
	"""C = alpha * A @ B (+ beta * cin) in fp64 on the matrix cores, arbitrary strides."""
	_dev(A, B)
	if A.dtype != torch.float64 or B.dtype != torch.float64:
		raise TypeError("gemm_f64 takes float64 tensors")
	M, K = A.shape
	K2, N = B.shape
	if K != K2:
		raise ValueError(f"gemm_f64: inner dimensions differ ({K} vs {K2})")
	if out is None:
		out = torch.empty((M, N), dtype=torch.float64, device=A.device)
	check(_lib.load().anncur_gemm_f64(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(out), out.stride(0), out.stride(1),
									  M, N, K, float(alpha), float(beta), _p(cin) if cin is not None else None,
									  cin.stride(0) if cin is not None else 0, cin.stride(1) if cin is not None else 0, _stream()), "gemm_f64")
	return out


_DT64 = {torch.float32: F32, torch.bfloat16: BF16, torch.float64: _lib.F64}


@_on_device
def convert_f64(src, dst, alpha=1.0, divide_by=None):
	"""dst[i, j] = (alpha * src[i, j]) / divide_by[0] in fp64: the product rounded, then the division rounded (alpha * src[i, j] without a
	divisor); f32 / bf16 / f64 -> f64, or f64 -> f32 (one more rounding, to nearest even); any strides."""
	_dev(src, dst)
	if tuple(src.shape) != tuple(dst.shape) or src.dim() != 2:
		raise ValueError("convert_f64: 2-D tensors of equal shape")
	check(_lib.load().anncur_convert_f64(_p(src), _DT64[src.dtype], src.stride(0), src.stride(1), _p(dst), _DT64[dst.dtype], dst.stride(0), dst.stride(1),
										 src.shape[0], src.shape[1], float(alpha), _p(divide_by) if divide_by is not None else None, _stream()), "convert_f64")
	return dst


@_on_device
def diff_sumsq_f64(X, Y=None, out=None):
	"""-> device tensor [sum (X - Y)^2, sum X^2] (float64, no host sync); X, Y contiguous float64 of equal size."""
	_dev(X)
	if X.dtype != torch.float64 or not X.is_contiguous() or (Y is not None and (Y.dtype != torch.float64 or not Y.is_contiguous() or Y.numel() != X.numel())):
		raise ValueError("diff_sumsq_f64: contiguous float64 tensors of equal size")
	out = torch.empty(2, dtype=torch.float64, device=X.device) if out is None else out
	check(_lib.load().anncur_diff_sumsq_f64(_p(X), _p(Y) if Y is not None else None, X.numel(), _p(out), _stream()), "diff_sumsq_f64")
	return out


@_on_device
def approx_error(X, Et, A_exact):
	"""Per-row sum_i (X.E - A)^2 and sum_i A^2 without materialising X.E
	(reference: eval/run_retrieval_eval_wrt_exact_crossenc.py:146-147)."""
	_dev(X, Et, A_exact)
	X, Et, A_exact = _rowmajor(X), _rowmajor(Et), _rowmajor(A_exact)
	Q, K = X.shape
	I = Et.shape[0]
	if Et.shape[1] != K or tuple(A_exact.shape) != (Q, I):
		raise ValueError("approx_error: shape mismatch")
	err = torch.empty(Q, dtype=torch.float32, device=X.device)
	nrm = torch.empty(Q, dtype=torch.float32, device=X.device)
	lib = _lib.load()
	step = 65535 * 128
	for q0 in range(0, Q, step):
		q1 = min(Q, q0 + step)
		check(lib.anncur_approx_error(_p(X[q0:q1]), _dt(X), _ld(X), _p(Et), _dt(Et), _ld(Et), _p(A_exact[q0:q1]), _dt(A_exact),
									  _ld(A_exact), q1 - q0, I, K, _p(err[q0:q1]), _p(nrm[q0:q1]), _stream()), "approx_error")
	return err, nrm


def approx_error_packed_ok(Kp, A_exact):
	"""True if anncur_approx_error_packed takes these operands (bf16 MFMA loop of the sweep instead of the strided fp32 GEMM)."""
	return (Kp in (64, 128, 256, 512) and A_exact.dim() == 2 and A_exact.stride(1) == 1 and _ld(A_exact) % 4 == 0
			and _ld(A_exact) >= A_exact.shape[1] and A_exact.data_ptr() % 16 == 0)


@_on_device
def approx_error_packed(Xp, Etp, A_exact, n_items):
	"""a11 on the fused path's operands: Xp [Q x Kp] packed bf16, Etp [ceil32(I) x Kp] packed bf16, A_exact [Q x I] fp32 / bf16."""
	_dev(Xp, Etp, A_exact)
	Q, Kp = Xp.shape
	if Etp.shape[1] != Kp or tuple(A_exact.shape) != (Q, n_items) or Etp.shape[0] < (n_items + 31) // 32 * 32:
		raise ValueError("approx_error_packed: shape mismatch")
	if Xp.dtype != torch.bfloat16 or Etp.dtype != torch.bfloat16 or not approx_error_packed_ok(Kp, A_exact):
		raise ValueError("approx_error_packed: operands must be packed bf16 and the exact matrix 16-byte aligned with a row pitch multiple of 4")
	err = torch.empty(Q, dtype=torch.float32, device=Xp.device)
	nrm = torch.empty(Q, dtype=torch.float32, device=Xp.device)
	check(_lib.load().anncur_approx_error_packed(_p(Xp), _ld(Xp), _p(Etp), _ld(Etp), _p(A_exact), _dt(A_exact), _ld(A_exact), Q, n_items, Kp,
												 _p(err), _p(nrm), _stream()), "approx_error_packed")
	return err, nrm


def eval_fused_ok(Kp, A_exact, Q, I, k):
	"""True if anncur_eval_fused takes this cell: Kp <= 256, bf16 exact matrix with 16-byte aligned rows, shape inside the fused path."""
	if not (Kp in (64, 128, 256) and A_exact.dim() == 2 and A_exact.dtype == torch.bfloat16 and A_exact.stride(1) == 1 and _ld(A_exact) % 8 == 0
			and _ld(A_exact) >= A_exact.shape[1] and A_exact.data_ptr() % 16 == 0):
		return False
	# the kernel's exact-tile offsets are 32-bit (255 rows x pitch x 2 bytes, csrc/score_fused.hip exact_tile_offsets_fit): longer pitches take the two-kernel route
	if 255 * _ld(A_exact) * 2 + 64 >= 1 << 32:
		return False
	# one workspace for the whole cell (no query chunks here): cells above the limit take the chunked two-kernel route
	nbytes = _lib.load().anncur_eval_fused_workspace_bytes(Q, I, Kp, k)
	return 0 < nbytes <= FUSED_WS_LIMIT_BYTES


@_on_device
def eval_fused(Xp, Etp, A_exact, n_items, k, return_fallbacks=False, hint=None):
	"""One sweep for a grid cell of entry point A (reference: eval/run_retrieval_eval_wrt_exact_crossenc.py:84,106,146-147):
	(TopK of S_hat = Xp . Etp^T, err_sq [Q], norm_sq [Q]).  Xp [Q x Kp], Etp [ceil32(I) x Kp] packed bf16 in ITEM order, A_exact [Q x I] bf16.
	hint: a copy of Etp's rows in descending-norm order (same shape): the prepass samples ITS leading tiles -- a tighter first threshold, same results."""
	_dev(Xp, Etp, A_exact)
	Q, Kp = Xp.shape
	if Xp.dtype != torch.bfloat16 or Etp.dtype != torch.bfloat16 or Etp.shape[1] != Kp or not Etp.is_contiguous() or Etp.shape[0] < -(-n_items // 32) * 32 \
			or tuple(A_exact.shape) != (Q, n_items):
		raise ValueError("eval_fused: Xp [Q x Kp], Etp [ceil32(I) x Kp] packed bf16, A_exact [Q x I]")
	if not eval_fused_ok(Kp, A_exact, Q, n_items, k):
		raise _lib.AnncurHipError(f"eval_fused: cell (Q={Q}, I={n_items}, Kp={Kp}, k={k}, A {A_exact.dtype}) is outside the one-pass route")
	Xp = _rowmajor(Xp)
	lib = _lib.load()
	nbytes = lib.anncur_eval_fused_workspace_bytes(Q, n_items, Kp, k)
	ws = _Workspace.get(nbytes, Xp.device)
	val = torch.empty((Q, k), dtype=torch.float32, device=Xp.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=Xp.device)
	err = torch.empty(Q, dtype=torch.float32, device=Xp.device)
	nrm = torch.empty(Q, dtype=torch.float32, device=Xp.device)
	if hint is not None:
		_dev(hint)
		if hint.dtype != torch.bfloat16 or tuple(hint.shape) != tuple(Etp.shape) or not hint.is_contiguous():
			raise ValueError("eval_fused: hint must be a contiguous bf16 copy of Etp's rows (same shape)")
	check(lib.anncur_eval_fused_ex(_p(Xp), _ld(Xp), _p(Etp), Kp, _p(hint) if hint is not None else None, _p(A_exact), _dt(A_exact), _ld(A_exact), Q, n_items, Kp, k,
								   _p(val), _p(idx), _p(err), _p(nrm), _p(ws), nbytes, _stream()), "eval_fused")
	if return_fallbacks:
		return TopK(val, idx), err, nrm, ws[:4].view(torch.int32)
	return TopK(val, idx), err, nrm


# ------------------------------------------------------------------ a7/a8
@_on_device
def rowwise_topk(A, k, out=None, _spec=None, _stats=None):
	"""Exact torch.topk(A, k, dim=1) on the device: (values f32 [Q,k], indices int32 [Q,k]),
	sorted descending, ties -> smaller index.  out: (values, indices) contiguous [Q, k] tensors to write into (row slices of a larger
	result, when a matrix is scanned in several launches).
	_spec / _stats (tests and measurements; anncur_rowwise_topk_ex): rank of the wave-per-row scan's speculative start -- None = the
	library's choice, 0 = off, 1..k forced -- and a zeroed int32 [2] device tensor the launch adds (rows scanned twice, rows started from a
	guess) to.  The result does not depend on either."""
	_dev(A)
	A = _rowmajor(A)
	Q, I = A.shape
	if out is not None:
		val, idx = out
		if tuple(val.shape) != (Q, k) or tuple(idx.shape) != (Q, k) or val.dtype != torch.float32 or idx.dtype != torch.int32 or not val.is_contiguous() or not idx.is_contiguous():
			raise ValueError("rowwise_topk: out must be contiguous (float32 [Q, k], int32 [Q, k])")
	else:
		val = torch.empty((Q, k), dtype=torch.float32, device=A.device)
		idx = torch.empty((Q, k), dtype=torch.int32, device=A.device)
	if _spec is None and _stats is None:
		check(_lib.load().anncur_rowwise_topk(_p(A), _dt(A), Q, I, _ld(A), k, _p(val), _p(idx), _stream()), "rowwise_topk")
		return TopK(val, idx)
	if _stats is not None:
		_dev(_stats)
		if _stats.dtype != torch.int32 or _stats.numel() < 2 or not _stats.is_contiguous():
			raise ValueError("rowwise_topk: _stats must be a contiguous int32 tensor of two entries")
	check(_lib.load().anncur_rowwise_topk_ex(_p(A), _dt(A), Q, I, _ld(A), k, _p(val), _p(idx), _stream(), -1 if _spec is None else int(_spec),
											 _p(_stats) if _stats is not None else None), "rowwise_topk")
	return TopK(val, idx)


@_on_device
def rowwise_topk_ragged(A, row_len, k):
	"""rowwise_topk over ragged rows: row q of A holds row_len[q] (int32 tensor, k <= row_len[q] <= A.shape[1]) elements; k <= 128."""
	_dev(A, row_len)
	A = _rowmajor(A)
	Q, I = A.shape
	if row_len.dtype != torch.int32 or row_len.numel() != Q or not row_len.is_contiguous():
		raise ValueError("rowwise_topk_ragged: row_len must be a contiguous int32 tensor with one entry per row")
	val = torch.empty((Q, k), dtype=torch.float32, device=A.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=A.device)
	check(_lib.load().anncur_rowwise_topk_ragged(_p(A), _dt(A), Q, I, _ld(A), _p(row_len), k, _p(val), _p(idx), _stream()), "rowwise_topk_ragged")
	return TopK(val, idx)


GatherTables = namedtuple("GatherTables", ["col_idx", "vec_tab", "n_items", "dtype"])


@_on_device
def gather_tables(col_idx, n_items, dtype):
	"""The per-anchor-set tables of rowwise_topk_gather: col_idx ascending, distinct columns (int32 / int64 tensor on the GPU)."""
	_dev(col_idx)
	if col_idx.dim() != 1 or col_idx.numel() < 1 or col_idx.numel() > 65535:
		raise ValueError("gather_tables: 1..65535 anchor columns")
	ci = col_idx.to(torch.int32).contiguous()
	if bool((ci[1:] <= ci[:-1]).any()) or int(ci[0]) < 0 or int(ci[-1]) >= n_items:
		raise ValueError("gather_tables: columns must be ascending, distinct and inside the matrix")
	vec = 8 if dtype == torch.bfloat16 else 4
	n_vec = -(-n_items // vec)
	tab = torch.empty(n_vec, dtype=torch.int32, device=ci.device)
	check(_lib.load().anncur_gather_tables(_p(ci), ci.numel(), n_items, BF16 if dtype == torch.bfloat16 else F32, _p(tab), _stream()), "gather_tables")
	return GatherTables(ci, tab, n_items, dtype)


def rowwise_topk_gather_ok(A, k):
	"""True if rowwise_topk_gather takes this matrix: wave-level scan (k <= 128), 16-byte aligned rows."""
	return (k <= 128 and A.dim() == 2 and A.stride(1) == 1 and A.data_ptr() % 16 == 0
			and (A.shape[0] == 1 or (_ld(A) * A.element_size()) % 16 == 0) and A.dtype in (torch.float32, torch.bfloat16))


@_on_device
def rowwise_topk_gather(A, k, tables, out=None, cq_out=None):
	"""rowwise_topk(A, k) and C_q = A[:, tables.col_idx] from ONE pass over A (reference: the slice test_scores[:, anchor_ent_idxs] of
	..._splits.py:297,300 folded into the exact top-k of :86).  Returns (TopK, C_q [Q x n_idx] of A's dtype)."""
	_dev(A)
	A = _rowmajor(A)
	Q, I = A.shape
	if tables.n_items != I or tables.dtype != A.dtype or not rowwise_topk_gather_ok(A, k):
		raise ValueError("rowwise_topk_gather: tables built for another matrix shape / dtype, k > 128, or rows not 16-byte aligned")
	n_idx = tables.col_idx.numel()
	if out is not None:
		val, idx = out
		if (tuple(val.shape) != (Q, k) or tuple(idx.shape) != (Q, k) or val.dtype != torch.float32 or idx.dtype != torch.int32
				or not val.is_contiguous() or not idx.is_contiguous() or val.device != A.device or idx.device != A.device):
			raise ValueError("rowwise_topk_gather: out must be contiguous (float32 [Q, k], int32 [Q, k]) on A's device")
	else:
		val = torch.empty((Q, k), dtype=torch.float32, device=A.device)
		idx = torch.empty((Q, k), dtype=torch.int32, device=A.device)
	cq = cq_out if cq_out is not None else torch.empty((Q, n_idx), dtype=A.dtype, device=A.device)
	if tuple(cq.shape) != (Q, n_idx) or cq.dtype != A.dtype or (n_idx > 1 and cq.stride(1) != 1) or cq.device != A.device or (Q > 1 and cq.stride(0) < n_idx):
		raise ValueError("rowwise_topk_gather: cq_out must be [Q x n_idx] of A's dtype on A's device, unit column stride")
	check(_lib.load().anncur_rowwise_topk_gather(_p(A), _dt(A), Q, I, _ld(A), k, _p(val), _p(idx), _p(tables.col_idx), n_idx,
												  _p(tables.vec_tab), _p(cq), _ld(cq), _stream()), "rowwise_topk_gather")
	return TopK(val, idx), cq


_KP_CHOICES = (64, 128, 256, 512)   # query operand resident in registers (score_sweep_kernel)
_KP_WIDE_MAX = 4096                  # beyond: LDS-tiled K-general kernel (wide_kernel), Kp a multiple of 128


def padded_k(K):
	"""Inner dimension the fused kernels take for a logical K (zero-padded), or None if K is too wide for them."""
	for kp in _KP_CHOICES:
		if K <= kp:
			return kp
	kp = -(-K // 128) * 128
	return kp if kp <= _KP_WIDE_MAX else None


def _kp_ok(Kp):
	return Kp in _KP_CHOICES or (512 < Kp <= _KP_WIDE_MAX and Kp % 128 == 0)


@_on_device
def pack_bf16(M, Kp, row_multiple=1):
	"""[n x K] (f32/bf16) -> zero-padded bf16 [ceil(n/row_multiple)*row_multiple x Kp], packed."""
	_dev(M)
	n, K = M.shape
	n_pad = -(-n // row_multiple) * row_multiple
	out = torch.zeros((n_pad, Kp), dtype=torch.bfloat16, device=M.device)
	M = _rowmajor(M)
	view = out[:n, :K]
	check(_lib.load().anncur_convert(_p(M), _dt(M), _ld(M), _p(view), BF16, Kp, n, K, _stream()), "pack_bf16")
	return out


def split_kp(K):
	"""Inner dimension of the split-bf16 ("bf16x3") operands for a logical K: padded_k(3 K) -- three K-wide segments per row --, or None."""
	return padded_k(3 * K)


@_on_device
def pack_split_bf16(M, role, Kp=None, row_multiple=1, out=None):
	"""[n x K] (f32/bf16) -> bf16 [ceil(n/row_multiple)*row_multiple x Kp] split operand of the bf16x3 route: with hi = bf16(x) and
	lo = bf16(x - hi), role 0 (queries) holds [lo | hi | hi | 0], role 1 (items) [hi | lo | hi | 0], so that a row of one times a row of
	the other is lo.hi + hi.lo + hi.hi.  Kp defaults to split_kp(K).  The kernel writes the zero padding itself (no memset).
	out: a contiguous bf16 [n_pad x Kp] tensor to fill (every element is overwritten)."""
	_dev(M)
	n, K = M.shape
	if role not in (0, 1):
		raise ValueError("pack_split_bf16: role is 0 (query rows) or 1 (item rows)")
	if Kp is None:
		Kp = split_kp(K)
	if Kp is None or Kp < 3 * K or Kp % 8 != 0 or K < 1:
		raise ValueError(f"pack_split_bf16: K = {K} does not fit Kp = {Kp} (need 1 <= 3 K <= Kp, Kp a multiple of 8)")
	n_pad = -(-n // row_multiple) * row_multiple
	if out is None:
		out = torch.empty((n_pad, Kp), dtype=torch.bfloat16, device=M.device)
	elif tuple(out.shape) != (n_pad, Kp) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != M.device:
		raise ValueError("pack_split_bf16: out must be a contiguous bf16 [n_pad x Kp] tensor on M's device")
	M = _rowmajor(M)
	check(_lib.load().anncur_pack_split_bf16(_p(M), _dt(M), _ld(M), n, K, role, _p(out), Kp, n_pad, _stream()), "pack_split_bf16")
	return out


@_on_device
def rescore_topk(X, Et, cand_idx, k_out):
	"""The k_out best of each query's candidates by the TRUE fp32 score: for i in cand_idx[q] (int32 [Q x n_cand], distinct; < 0 or
	>= I: a hole) s = the k-ordered fp32 fmaf chain of <X[q], Et[i]> -- bit for bit the element gemm(X, Et.t()) holds --, then
	TopK(values f32 [Q x k_out], item ids int32) by score descending, ties by the smaller id, padded with (-inf, -1).
	(reference: the scores eval/matrix_approx_zeshel.py:118,126 and models/nearest_nbr.py:36-38 rank by.)"""
	_dev(X, Et, cand_idx)
	X, Et = _rowmajor(X), _rowmajor(Et)
	if cand_idx.dim() != 2 or cand_idx.dtype != torch.int32 or (cand_idx.shape[1] > 1 and cand_idx.stride(1) != 1):
		cand_idx = cand_idx.to(torch.int32).contiguous()
	Q, K = X.shape
	I = Et.shape[0]
	n_cand = cand_idx.shape[1]
	if Et.shape[1] != K or cand_idx.shape[0] != Q:
		raise ValueError("rescore_topk: X [Q x K], Et [I x K], cand_idx [Q x n_cand]")
	val = torch.empty((Q, k_out), dtype=torch.float32, device=X.device)
	idx = torch.empty((Q, k_out), dtype=torch.int32, device=X.device)
	scratch = _ScoreScratch.get(max(Q * n_cand, 1), X.device)
	check(_lib.load().anncur_rescore_topk(_p(X), _dt(X), _ld(X), _p(Et), _dt(Et), _ld(Et), K, _p(cand_idx), _ld(cand_idx), n_cand, Q, I, k_out,
										  _p(val), _p(idx), _p(scratch), _stream()), "rescore_topk")
	return TopK(val, idx)


SPLIT_RESCORE_EXTRA = 16   # candidates the bf16x3 sweep retrieves beyond k before the fp32 rescore: max(this, k // 8) (DESIGN 4.4a has the table)


def split_rescore_extra(k):
	return max(SPLIT_RESCORE_EXTRA, k // 8)


def split_candidates(I, k, extra=None, n_excl=0):
	"""Candidates per query the bf16x3 sweep retrieves for a final top-k of k: min(I, MAX_TOPK, k + extra); with an exclusion of at most
	n_excl items per query, min(I, MAX_TOPK, k + n_excl + extra) -- the margin `extra` still belongs to k."""
	return min(I, _lib.MAX_TOPK, k + n_excl + (split_rescore_extra(k) if extra is None else extra))


@_on_device
def score_topk_split(X, Et_f32, Etp_split, I, k, item_ids=None, leading_sample=False, extra=None, exclude=None):
	"""The bf16x3 route: top-k of S_hat = X.E at fp32 parity without writing S_hat.  X [Q x K] (f32/bf16), Et_f32 [I x K] the item
	embeddings in ITEM order, Etp_split = pack_split_bf16(rows of Et_f32, role 1, row_multiple=32), its rows in item order or -- with
	item_ids / leading_sample as for score_topk_fused -- in the index builder's order.  The fused sweep retrieves
	kc = min(I, MAX_TOPK, k + extra) candidates on the split operands (scores within (2^-16 + 3K 2^-23) |X|.|E|^T of exact), rescore_topk
	ranks them by the true fp32 score: values bit-equal to the dense fp32 route's.  Raises where the shape is outside the fused path.
	exclude: an Exclusion (exclusion()): the sweep retrieves e_max more candidates, filter_topk keeps the first k + extra allowed ones --
	the top k + extra by split score among the allowed items -- and the rescore ranks those."""
	_dev(X, Et_f32, Etp_split)
	Q, K = X.shape
	Kp = Etp_split.shape[1]
	e = exclude.e_max if exclude is not None else 0
	kc = split_candidates(I, k, extra, e)
	if Kp < 3 * K or Et_f32.shape[0] != I or Et_f32.shape[1] != K or k + e > kc:
		raise ValueError("score_topk_split: X [Q x K], Et_f32 [I x K], Etp_split [ceil32(I) x Kp >= 3 K], k (+ excluded per query) <= min(I, MAX_TOPK)")
	if not fused_supported(Q, I, Kp, kc):
		raise _lib.AnncurHipError(f"score_topk_split: shape (Q={Q}, I={I}, Kp={Kp}, k={kc}) is outside the fused path")
	cand = score_topk_fused(pack_split_bf16(X, 0, Kp), Etp_split, I, kc, leading_sample=leading_sample, item_ids=item_ids)
	if e:
		cand = filter_topk(cand.values, cand.indices, exclude, min(kc, split_candidates(I, k, extra)))
	return rescore_topk(X, Et_f32, cand.indices, k)


# ------------------------------------------------------------------ filtered retrieval
Exclusion = namedtuple("Exclusion", ["off", "ids", "e_max"])


def _sorted_unique_ids(a, I, what, pad=False):
	"""One exclusion list -> sorted, distinct int64 numpy ids; pad: -1 entries are padding and dropped."""
	a = np.asarray(a)
	if a.ndim != 1:
		raise ValueError(f"exclude: {what} must be a flat list of item ids")
	if a.size and not np.issubdtype(a.dtype, np.integer):
		if not np.issubdtype(a.dtype, np.floating) or not np.array_equal(a, np.floor(a)):
			raise ValueError(f"exclude: {what} must hold integer item ids")
	a = a.astype(np.int64)
	if pad:
		a = a[a != -1]
	if a.size:
		lo, hi = int(a.min()), int(a.max())
		if lo < 0:
			raise ValueError(f"exclude: {what} holds the negative id {lo}" + (" (only -1 pads a 2-D array)" if pad else ""))
		if I is not None and hi >= I:
			raise ValueError(f"exclude: {what} holds the id {hi}, but there are only {I} items")
		if hi > 0x7fffffff:
			raise ValueError(f"exclude: {what} holds the id {hi}, beyond int32")
	return np.unique(a)


def _host_array(x):
	return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def exclusion(exclude, Q, I, device):
	"""The `exclude=` argument of the top-k calls -> Exclusion(off, ids, e_max) for anncur_filter_topk: ids int32 on `device`, each
	list sorted and de-duplicated; off int64 [Q + 1] on `device` (per-query lists, segment q = ids[off[q]:off[q + 1]]) or None (one
	list shared by all queries); e_max = the longest list.  Accepted:
	  * a flat sequence / 1-D array / 1-D tensor of ids: shared by all queries;
	  * a sequence of Q sequences (lists, arrays, tensors), one per query;
	  * a 2-D [Q x w] integer array or tensor, rows padded with -1.
	ValueError: an id >= I (I None: not checked), a negative id other than the 2-D form's -1 padding, a wrong number of lists.
	An Exclusion passes through (its Q is checked), so an index can normalise a fixed set -- its anchor items -- once and reuse it:
	lists given as GPU tensors are copied to the host here, a synchronisation."""
	device = torch.device(device)
	if isinstance(exclude, Exclusion):
		if exclude.off is not None and exclude.off.numel() != Q + 1:
			raise ValueError(f"exclude: the exclusion was built for {exclude.off.numel() - 1} queries, the call has {Q}")
		return exclude
	if exclude is None:
		return Exclusion(None, None, 0)
	x = _host_array(exclude)
	per_query = None
	if isinstance(x, np.ndarray):
		if x.ndim == 1:
			shared = _sorted_unique_ids(x, I, "the shared list")
		elif x.ndim == 2:
			if x.shape[0] != Q:
				raise ValueError(f"exclude: the 2-D array has {x.shape[0]} rows, the call has {Q} queries")
			per_query = [_sorted_unique_ids(r, I, f"row {q}", pad=True) for q, r in enumerate(x)]
		else:
			raise ValueError("exclude: an array must be 1-D (shared) or 2-D [Q x w] (-1 padded)")
	else:
		x = list(x)
		if any(torch.is_tensor(r) or isinstance(r, (list, tuple, np.ndarray, range)) for r in x):
			if len(x) != Q:
				raise ValueError(f"exclude: {len(x)} per-query lists, the call has {Q} queries")
			per_query = [_sorted_unique_ids(_host_array(r), I, f"list {q}") for q, r in enumerate(x)]
		else:
			shared = _sorted_unique_ids(np.asarray(x) if x else np.zeros(0, dtype=np.int64), I, "the shared list")
	if per_query is None:
		return Exclusion(None, torch.from_numpy(shared.astype(np.int32)).to(device), int(shared.size))
	lens = np.array([r.size for r in per_query], dtype=np.int64)
	off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
	ids = np.concatenate(per_query).astype(np.int32) if per_query else np.zeros(0, dtype=np.int32)
	return Exclusion(torch.from_numpy(off).to(device), torch.from_numpy(ids).to(device), int(lens.max(initial=0)))


def filtered_k(k, e_max, I):
	"""Candidates per query a top-k asks for when up to e_max items per query are excluded: kc = k + e_max, because the unfiltered
	top-(k + e) contains the filtered top-k.  ValueError beyond what one top-k call returns."""
	kc = k + e_max
	limit = min(I, _lib.MAX_TOPK)
	if kc > limit:
		raise ValueError(f"exclude: k + the longest exclusion list = {k} + {e_max} = {kc} candidates per query, above the limit of min(items, ANNCUR_MAX_TOPK) = "
						 f"min({I}, {_lib.MAX_TOPK}) = {limit} of one top-k call; to exclude a set this large, rebuild the index without those items")
	return kc


@_on_device
def filter_topk(val, idx, exclude, k_out):
	"""The first k_out entries of each row of (val f32 [Q x n_cand], idx int32 [Q x n_cand]) -- a top-k result: descending, id < 0 a
	hole -- that are neither holes nor excluded, in the row's order, padded with (-inf, -1).  exclude: anything exclusion() takes
	(ids are not checked against an item count here)."""
	_dev(val, idx)
	if val.dim() != 2 or tuple(val.shape) != tuple(idx.shape):
		raise ValueError("filter_topk: val and idx must be 2-D tensors of one shape")
	if val.dtype != torch.float32:
		raise TypeError("filter_topk takes float32 scores")
	if idx.dtype != torch.int32:
		idx = idx.to(torch.int32)
	val, idx = _rowmajor(val), _rowmajor(idx)
	if _ld(val) != _ld(idx):
		val, idx = val.contiguous(), idx.contiguous()
	Q, n_cand = val.shape
	ex = exclusion(exclude, Q, None, val.device)
	out_val = torch.empty((Q, k_out), dtype=torch.float32, device=val.device)
	out_idx = torch.empty((Q, k_out), dtype=torch.int32, device=val.device)
	n_ids = ex.ids.numel() if ex.ids is not None else 0
	if Q == 0:
		return TopK(out_val, out_idx)
	check(_lib.load().anncur_filter_topk(_p(val), _p(idx), _ld(val), n_cand, Q, _p(ex.off) if ex.off is not None else None,
										 _p(ex.ids) if n_ids else None, n_ids if ex.off is None else 0, k_out, _p(out_val), _p(out_idx), _stream()), "filter_topk")
	return TopK(out_val, out_idx)


FUSED_WS_LIMIT_BYTES = 32 << 30   # default workspace above this size -> score_topk_fused runs the queries in row chunks


def _aligned_bytes(n, device, buf=None):
	"""A 256-byte aligned uint8 tensor of n bytes: freshly allocated, or inside `buf` (uint8, n + 256 bytes or more)."""
	if buf is None:
		buf = torch.empty(n + 256, dtype=torch.uint8, device=device)
	off = (-buf.data_ptr()) % 256
	return buf[off:off + n]


class _Scratch:
	"""Grow-only device scratch: one buffer per device in each subclass' own _bufs (the subclasses never share memory).  A byte scratch
	hands out 256-byte aligned views and keeps 256 bytes of room for that; an element scratch hands out the buffer's front."""
	_dtype, _room = torch.uint8, 256

	@classmethod
	def get(cls, n, device):
		key = (device.type, device.index)
		buf = cls._bufs.get(key)
		if buf is None or buf.numel() < n + cls._room:
			cls._bufs[key] = buf = torch.empty(n + cls._room, dtype=cls._dtype, device=device)
		return _aligned_bytes(n, device, buf) if cls._room else buf[:n]


class _Workspace(_Scratch):
	"""The fused kernels' workspace."""
	_bufs = {}


class _ScoreScratch(_Scratch):
	"""fp32 elements: the batched IVF searches' score matrix."""
	_bufs = {}
	_dtype, _room = torch.float32, 0


class _ByteScratch(_Scratch):
	"""The workspace of ivf_search_grouped."""
	_bufs = {}


def fused_supported(Q, I, Kp, k):
	return _kp_ok(Kp) and bool(_lib.load().anncur_score_topk_supported(Q, I, Kp, k))


def fused_workspace(Q, I, Kp, k, device):
	"""A private workspace for score_topk_fused (256-byte aligned uint8 tensor): calls that may run concurrently on different
	streams must not share the default one."""
	nbytes = _lib.load().anncur_score_topk_workspace_bytes(Q, I, Kp, k)
	if nbytes == 0:
		raise _lib.AnncurHipError(f"score_topk: shape (Q={Q}, I={I}, Kp={Kp}, k={k}) is outside the fused path")
	return _aligned_bytes(nbytes, device)


def _item_ids_arg(item_ids, I, device):
	if item_ids is None:
		return None
	if item_ids.dtype != torch.int32 or item_ids.numel() != I or not item_ids.is_contiguous() or item_ids.device != device:
		raise ValueError("item_ids must be a contiguous int32 device tensor with one id per item")
	return item_ids


def _topk_flags(leading_sample=False, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""The flags word of anncur_score_topk_ex / _timed / _plan_ex."""
	return ((_lib.TOPK_LEADING_SAMPLE if leading_sample else 0) | (_lib.TOPK_MFMA16 if mfma16 else 0) | (_lib.TOPK_QT1 if qt1 else 0)
			| (_lib.TOPK_MFMA32 if mfma32 else 0) | (_lib.TOPK_RING if ring else 0) | (_lib.TOPK_STAGED if staged else 0))


@_on_device
def score_topk_fused(Xp, Etp, I, k, return_fallbacks=False, workspace=None, leading_sample=False, item_ids=None, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""Fused S_hat = X.E + top-k.  Xp [Q x Kp] bf16 packed, Etp [Ip x Kp] bf16 packed (see pack_bf16).
	workspace: from fused_workspace(); default = one grow-only buffer per device (one call in flight at a time).
	leading_sample / item_ids: the index builder's hints of anncur_score_topk_ex (rows of Etp ordered by descending norm, and the
	map from rows back to item ids); the result is the exact top-k either way.
	mfma16 / mfma32 / qt1: the sweep variants ANNCUR_TOPK_MFMA16 / _MFMA32 / _QT1 (fused_plan(..., mfma16=, ...) tells whether the shape
	takes them: "lg" == 1 / "lg" == 2 / "QT" == 1; the default for Kp <= 256 is the 16x16x32 body with its threshold ladder up to k = 1024,
	32x32x16 above; staged=True runs the sweep in stages without the ladder, on the 16x16x32 body up to k = 384 and on 32x32x16 above)."""
	_dev(Xp, Etp)
	if Xp.dtype != torch.bfloat16 or Etp.dtype != torch.bfloat16:
		raise TypeError("score_topk_fused takes bf16 operands")
	Q, Kp = Xp.shape
	if Etp.shape[1] != Kp or not Etp.is_contiguous() or Etp.shape[0] < -(-I // 32) * 32:
		raise ValueError("Et must be packed [ceil(I/32)*32 x Kp]")
	Xp = _wide_queries(_rowmajor(Xp))
	lib = _lib.load()
	nbytes = lib.anncur_score_topk_workspace_bytes(Q, I, Kp, k)
	if nbytes == 0:
		raise _lib.AnncurHipError(f"score_topk: shape (Q={Q}, I={I}, Kp={Kp}, k={k}) is outside the fused path")
	if workspace is None and nbytes > FUSED_WS_LIMIT_BYTES and Q > 512 and not return_fallbacks:
		# very many queries: the candidate segments grow with Q; run row chunks whose workspace stays under the limit
		qc = Q
		while qc > 512 and lib.anncur_score_topk_workspace_bytes(qc, I, Kp, k) > FUSED_WS_LIMIT_BYTES:
			qc = max(512, (qc // 2 + 255) // 256 * 256)
		val = torch.empty((Q, k), dtype=torch.float32, device=Xp.device)
		idx = torch.empty((Q, k), dtype=torch.int32, device=Xp.device)
		for q0 in range(0, Q, qc):   # (a chunk of 512 queries is accepted whatever its workspace size)
			part = score_topk_fused(Xp[q0:q0 + qc], Etp, I, k, leading_sample=leading_sample, item_ids=item_ids, mfma16=mfma16, qt1=qt1, mfma32=mfma32, ring=ring, staged=staged)
			val[q0:q0 + qc], idx[q0:q0 + qc] = part.values, part.indices
		return TopK(val, idx)
	if workspace is None:
		ws = _Workspace.get(nbytes, Xp.device)
	else:
		ws = workspace
		if ws.numel() < nbytes or ws.data_ptr() % 256 != 0 or ws.device != Xp.device:
			raise ValueError("score_topk_fused: workspace too small, misaligned or on another device (use fused_workspace())")
	val = torch.empty((Q, k), dtype=torch.float32, device=Xp.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=Xp.device)
	ids = _item_ids_arg(item_ids, I, Xp.device)
	check(lib.anncur_score_topk_ex(_p(Xp), _ld(Xp), _p(Etp), Kp, Q, I, Kp, k, _p(val), _p(idx), _p(ws), nbytes,
								   _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), _p(ids) if ids is not None else None, _stream()), "score_topk")
	if return_fallbacks:
		return TopK(val, idx), ws[:4].view(torch.int32)
	return TopK(val, idx)


# ------------------------------------------------------------------ small-batch route (csrc/few.hip)
FEW_MAX_Q = 64              # ANNCUR_FEW_MAX_Q
FEW_STAGE_BYTES = 65536     # ANNCUR_FEW_STAGE_BYTES
_FEW_PLAN = ("tiles", "workgroups", "waves_per_workgroup", "tiles_per_wave_min", "tiles_per_wave_max", "query_subtiles", "groups", "cand_cap",
			 "pitch", "groups_per_wave", "gmax_offset", "scores_offset")
FewStats = namedtuple("FewStats", ["groups_read", "n_cand", "fallback"])


def _few_check(what, Q, I, Kp, k=None):
	"""Host-side limits of the small-batch route; a ValueError names the one that is broken."""
	if not 1 <= Q <= FEW_MAX_Q:
		raise ValueError(f"{what}: Q = {Q} queries, the small-batch route takes 1..{FEW_MAX_Q} per call")
	if not _kp_ok(Kp):
		raise ValueError(f"{what}: Kp = {Kp} is not a padded inner dimension (64, 128, 256, 512 or a multiple of 128 up to {_KP_WIDE_MAX}: padded_k)")
	stage = 16 * -(-Q // 16) * Kp * 2
	if stage > FEW_STAGE_BYTES:
		raise ValueError(f"{what}: {-(-Q // 16) * 16} staged query rows of Kp = {Kp} take {stage} bytes, above the LDS stage of {FEW_STAGE_BYTES}")
	if not 1 <= I < (1 << 31) - 1:
		raise ValueError(f"{what}: I = {I} items is outside 1..2^31 - 2")
	if k is not None:
		limit = min(I, _lib.MAX_TOPK)
		if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= limit:
			raise ValueError(f"{what}: k = {k} outside 1..min(I, ANNCUR_MAX_TOPK) = min({I}, {_lib.MAX_TOPK}) = {limit}")


def _few_operands(what, Xp, Etp, I):
	"""Shape, dtype and pitch checks of the packed operands, before either has to be on the GPU -> (Q, Kp, ldx)."""
	if not (torch.is_tensor(Xp) and torch.is_tensor(Etp)) or Xp.dim() != 2 or Etp.dim() != 2:
		raise ValueError(f"{what}: Xp and Etp must be 2-D tensors")
	if Xp.dtype != torch.bfloat16 or Etp.dtype != torch.bfloat16:
		raise TypeError(f"{what} takes bf16 operands")
	Q, Kp = Xp.shape
	if Etp.shape[1] != Kp or not Etp.is_contiguous() or Etp.shape[0] < -(-I // 32) * 32:
		raise ValueError(f"{what}: Et must be packed [ceil(I/32)*32 x Kp]")
	if Kp > 1 and Xp.stride(1) != 1:
		raise ValueError(f"{what}: the rows of Xp must be contiguous")
	ldx = Xp.stride(0) if Q > 1 else max(Kp, 1)
	if ldx < Kp or ldx % 8 != 0:
		raise ValueError(f"{what}: ldx = {ldx}, the pitch of Xp must be >= Kp = {Kp} and a multiple of 8 (ldx % 8 == 0)")
	return Q, Kp, ldx


def score_topk_few_ok(Q, I, Kp, k):
	"""Does the small-batch route take the shape?  (host query, no GPU needed)"""
	return _kp_ok(Kp) and bool(_lib.load().anncur_score_topk_few_supported(Q, I, Kp, k))


def few_plan(Q, I, Kp, k):
	"""The plan of score_topk_few (host query): tiles of 16 items, workgroups, waves per workgroup, fewest / most tiles of a wave, 16-query
	sub-tiles, groups of 64 items per query, cand_cap (candidates the select buffers before it falls back to a full scan), the pitch of the
	score scratch in floats, groups per wave, byte offsets of the group maxima and the scores in the workspace."""
	_few_check("few_plan", Q, I, Kp, k)
	out = (ctypes.c_int32 * len(_FEW_PLAN))()
	check(_lib.load().anncur_score_topk_few_plan(Q, I, Kp, k, out, len(_FEW_PLAN)), "score_topk_few_plan")
	w = dict(zip(_FEW_PLAN, (int(x) for x in out)))
	w["pitch"] *= 32
	w["gmax_offset"] *= 256
	w["scores_offset"] *= 256
	return w


def few_workspace(Q, I, Kp, k, device):
	"""A private workspace for score_topk_few (256-byte aligned uint8 tensor), as fused_workspace."""
	_few_check("few_workspace", Q, I, Kp, k)
	nbytes = _lib.load().anncur_score_topk_few_workspace_bytes(Q, I, Kp, k)
	return _aligned_bytes(nbytes, device)


@_on_device
def score_topk_few(Xp, Etp, I, k, workspace=None, return_stats=False):
	"""Exact top-k of S_hat = X . E for 1..64 queries in two launches (csrc/few.hip): Xp [Q x Kp] bf16 (rows may be pitched, pitch a
	multiple of 8), Etp [ceil32(I) x Kp] bf16 packed in ITEM order (pack_bf16(..., row_multiple=32)).  Same result as score_topk_fused on the
	same operands, value bits included at Kp <= 256.  workspace: from few_workspace(); default = the grow-only buffer of the fused route.
	return_stats: also FewStats of int32 [Q] device tensors -- groups of 64 items the select read, candidates at or above its threshold,
	1 where it fell back to scanning the whole row.  Limits are checked on the host first (ValueError names the one that is broken)."""
	Q, Kp, ldx = _few_operands("score_topk_few", Xp, Etp, I)
	_few_check("score_topk_few", Q, I, Kp, k)
	_dev(Xp, Etp)
	lib = _lib.load()
	nbytes = lib.anncur_score_topk_few_workspace_bytes(Q, I, Kp, k)
	if workspace is None:
		ws = _Workspace.get(nbytes, Xp.device)
	else:
		ws = workspace
		if ws.numel() < nbytes or ws.data_ptr() % 256 != 0 or ws.device != Xp.device:
			raise ValueError("score_topk_few: workspace too small, misaligned or on another device (use few_workspace())")
	val = torch.empty((Q, k), dtype=torch.float32, device=Xp.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=Xp.device)
	check(lib.anncur_score_topk_few(_p(Xp), ldx, _p(Etp), Kp, Q, I, Kp, int(k), _p(val), _p(idx), _p(ws), nbytes, _stream()), "score_topk_few")
	if return_stats:
		h = ws[:16 * Q].view(torch.int32).view(Q, 4)
		return TopK(val, idx), FewStats(h[:, 0], h[:, 1], h[:, 2])
	return TopK(val, idx)


@_on_device
def score_rows_few(Xp, Etp, I):
	"""Launch 1 of score_topk_few alone ("get_complete_row for a few queries on the bf16 operands") -> (S [Q x I] fp32, a view of rows
	ceil32(I) apart, GM [Q x ceil(I / 64)] fp32: the maximum of every 64 consecutive items, NaN skipped, NaN for an all-NaN group)."""
	Q, Kp, ldx = _few_operands("score_rows_few", Xp, Etp, I)
	_few_check("score_rows_few", Q, I, Kp)
	_dev(Xp, Etp)
	pitch, G = -(-I // 32) * 32, -(-I // 64)
	S = torch.empty((Q, pitch), dtype=torch.float32, device=Xp.device)
	GM = torch.empty((Q, G), dtype=torch.float32, device=Xp.device)
	check(_lib.load().anncur_score_rows_few(_p(Xp), ldx, _p(Etp), Kp, Q, I, Kp, _p(S), pitch, _p(GM), G, _stream()), "score_rows_few")
	return S[:, :I], GM


_aux_streams = {}


def aux_stream(device):
	"""The second stream anncur_eval_topk forks the exact scan's row chunks onto (one per device, created on first use)."""
	key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
	if key not in _aux_streams:
		_aux_streams[key] = torch.cuda.Stream(device=device)
	return _aux_streams[key]


_cu_streams = {}


def cu_partition_streams(device, n_scan):
	"""Two streams that split the chip's compute units: (retrieval stream on the CUs the scan leaves, scan stream on `n_scan` CUs), by
	hipExtStreamCreateWithCUMask.  On MI355X the first n bits of the mask stand for n / 8 CUs on each of the 8 XCDs, in steps of 32
	bits (mapped in round 4 by reading XCC_ID / HW_ID per workgroup; sparse masks are ignored by the driver), so n_scan is rounded down to a multiple of 32.  For an
	HBM-bound kernel (the exact scan) beside an MFMA-bound one (the fused retrieval) whose workgroups fill the register file: sharing a
	CU means time-slicing it, a partition lets both run for the whole step.  Created once per (device, n_scan); fails loudly if the
	runtime lacks the call."""
	device = torch.device(device)
	idx = device.index if device.index is not None else torch.cuda.current_device()
	# hipExtStreamCreateWithCUMask makes BLOCKING streams: work on the NULL stream synchronises with them implicitly, and graph replays on a
	# masked stream right after NULL-stream work ended in a GPU memory access fault when RCCL was in the process (round 4; never
	# reproduced without RCCL: scripts/r5/cumask_null_stream_repro.hip).  A caller whose current stream is the NULL stream is one torch op away
	# from that: refused here.  Run under `with torch.cuda.stream(torch.cuda.Stream()):` (bench.py does).
	if torch.cuda.current_stream(idx).cuda_stream == 0:
		raise _lib.AnncurHipError("cu_partition_streams: the current stream is the NULL stream, which synchronises implicitly with CU-masked (blocking) streams; "
								  "make a non-default stream current first (with torch.cuda.stream(torch.cuda.Stream()): ...)")
	n_cu = torch.cuda.get_device_properties(idx).multi_processor_count
	n_scan = (int(n_scan) // 32) * 32
	if not (0 < n_scan < n_cu):
		raise ValueError(f"cu_partition_streams: n_scan={n_scan} must leave CUs on both sides of {n_cu}")
	key = (idx, n_scan)
	if key not in _cu_streams:
		hip = ctypes.CDLL("libamdhip64.so")
		fn = hip.hipExtStreamCreateWithCUMask
		fn.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
		words = (n_cu + 31) // 32
		def make(lo, hi):
			mask = (ctypes.c_uint32 * words)(*[sum(1 << b for b in range(32) if lo <= 32 * w + b < hi) for w in range(words)])
			h = ctypes.c_void_p()
			with torch.cuda.device(idx):
				rc = fn(ctypes.byref(h), words, mask)
			if rc != 0 or not h.value:
				raise _lib.AnncurHipError(f"hipExtStreamCreateWithCUMask failed (code {rc})")
			return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
		_cu_streams[key] = (make(n_scan, n_cu), make(0, n_scan))
	return _cu_streams[key]


@_on_device
def eval_topk(A, k, Xp, Etp, I, k_retvr, workspace=None, leading_sample=False, item_ids=None, mfma16=False, qt1=False, aux=None, serial=False, mfma32=False, ring=False, staged=False):
	"""The per-query evaluation loop's two top-k's in one call (reference: eval/run_retrieval_eval_wrt_exact_crossenc.py:97-106):
	(exact = rowwise_topk(A, k), approx = score_topk_fused(Xp, Etp, I, k_retvr)), the exact scan's row chunks co-scheduled with the
	retrieval's latency-bound launches on a second stream (anncur_eval_topk).  serial=True: the same two results, one after the other."""
	_dev(A, Xp, Etp)
	if Xp.dtype != torch.bfloat16 or Etp.dtype != torch.bfloat16:
		raise TypeError("eval_topk takes bf16 retrieval operands")
	A = _rowmajor(A)
	Q, Kp = Xp.shape
	if A.shape[0] != Q or A.shape[1] != I or Etp.shape[1] != Kp or not Etp.is_contiguous() or Etp.shape[0] < -(-I // 32) * 32:
		raise ValueError("eval_topk: A must be [Q x I], Et packed [ceil(I/32)*32 x Kp]")
	Xp = _wide_queries(_rowmajor(Xp))
	lib = _lib.load()
	nbytes = lib.anncur_score_topk_workspace_bytes(Q, I, Kp, k_retvr)
	if nbytes == 0:
		raise _lib.AnncurHipError(f"eval_topk: shape (Q={Q}, I={I}, Kp={Kp}, k={k_retvr}) is outside the fused path")
	ws = _Workspace.get(nbytes, Xp.device) if workspace is None else workspace
	if ws.numel() < nbytes or ws.data_ptr() % 256 != 0 or ws.device != Xp.device:
		raise ValueError("eval_topk: workspace too small, misaligned or on another device (use fused_workspace())")
	ev = torch.empty((Q, k), dtype=torch.float32, device=A.device)
	ei = torch.empty((Q, k), dtype=torch.int32, device=A.device)
	av = torch.empty((Q, k_retvr), dtype=torch.float32, device=A.device)
	ai = torch.empty((Q, k_retvr), dtype=torch.int32, device=A.device)
	ids = _item_ids_arg(item_ids, I, Xp.device)
	if serial:
		aux_p = None
	else:
		# (the chunks forked onto the auxiliary stream are joined back into the launch stream before the call returns: every tensor used
		#  there is ordered like launch-stream work, the caching allocator needs no record_stream)
		aux = aux or aux_stream(A.device)
		aux_p = ctypes.c_void_p(aux.cuda_stream)
	check(lib.anncur_eval_topk(_p(A), _dt(A), _ld(A), k, _p(ev), _p(ei), _p(Xp), _ld(Xp), _p(Etp), Kp, Q, I, Kp, k_retvr, _p(av), _p(ai), _p(ws), nbytes,
							   _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), _p(ids) if ids is not None else None, _stream(), aux_p), "eval_topk")
	return TopK(ev, ei), TopK(av, ai)


@_on_device
def score_topk_fused_timed(Xp, Etp, I, k, leading_sample=False, item_ids=None, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""Measurement only: (TopK, [prepass, threshold, sweep stage, select, sweep kernels only, n sweep launches, sweep launch 1, 2, 3]) in
	ms, from HIP events on the launch stream."""
	_dev(Xp, Etp)
	Q, Kp = Xp.shape
	Xp = _wide_queries(_rowmajor(Xp))
	lib = _lib.load()
	nbytes = lib.anncur_score_topk_workspace_bytes(Q, I, Kp, k)
	if nbytes == 0:
		raise _lib.AnncurHipError("score_topk_timed: unsupported shape")
	ws = _Workspace.get(nbytes, Xp.device)
	val = torch.empty((Q, k), dtype=torch.float32, device=Xp.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=Xp.device)
	ms = (ctypes.c_float * 9)()
	ids = _item_ids_arg(item_ids, I, Xp.device)
	check(lib.anncur_score_topk_timed(_p(Xp), _ld(Xp), _p(Etp), Kp, Q, I, Kp, k, _p(val), _p(idx), _p(ws), nbytes,
									  _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), _p(ids) if ids is not None else None, _stream(), ms),
		  "score_topk_timed")
	return TopK(val, idx), [float(x) for x in ms]


@_on_device
def fused_survivors(workspace, Q, I, Kp, k, leading_sample=False, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""Mean number of candidates per query the sweep of the last score_topk_fused call on `workspace` kept (diagnostics; synchronises)."""
	out = ctypes.c_double()
	check(_lib.load().anncur_score_topk_survivors(_p(workspace), Q, I, Kp, k, _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), ctypes.byref(out), _stream()),
		  "score_topk_survivors")
	return out.value


@_on_device
def fused_ladder_state(workspace, Q, I, Kp, k, leading_sample=False, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""The threshold ladder the sweep of the last score_topk_fused call on `workspace` (same shape and flags) left behind, as numpy arrays
	(diagnostics; synchronises): "levels" [Q x 8] float32 (ascending, above "tau0"), "counts" [Q x 8] uint32 (candidates counted with level
	j as the highest they reach: counts[:, j - 1]), "tau_final" [Q] float32 (the select's prefilter), "tau0" [Q] float32 (the prepass
	threshold).  Raises when the plan has no ladder (fused_plan(...)["ladder"] is False)."""
	levels = np.zeros((Q, 8), dtype=np.float32)
	counts = np.zeros((Q, 8), dtype=np.uint32)
	tau_final = np.zeros(Q, dtype=np.float32)
	tau0 = np.zeros(Q, dtype=np.float32)
	check(_lib.load().anncur_score_topk_ladder_state(_p(workspace), Q, I, Kp, k, _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged),
													  levels.ctypes.data, counts.ctypes.data, tau_final.ctypes.data, tau0.ctypes.data, _stream()),
		  "score_topk_ladder_state")
	return {"levels": levels, "counts": counts, "tau_final": tau_final, "tau0": tau0}


_PLAN_HEAD = ("n_sample_tiles", "n_tiles", "splits", "segment_capacity", "group", "lg", "QT", "n_stages")   # plan words 0..7


def _plan_words(out):
	"""The words of anncur_score_topk_plan_ex / anncur_eval_fused_plan by name, in the positions include/anncur_hip.h lists (enum PlanWord in
	csrc/score_fused.hip); words the call was not asked for read 0.  The per-stage arrays [3] are cut to the plan's stages."""
	v = [int(x) for x in out] + [0] * (27 - len(out))
	w = dict(zip(_PLAN_HEAD, v[:8]))
	n = w["n_stages"]
	w["stage_end"], w["stage_pred"], w["stage_flush"], w["stage_tiles_per_split"] = v[8:8 + n], v[11:11 + n], v[14:14 + n], v[24:24 + n]
	w["ladder"], w["ladder_top_rank"] = bool(v[17]), v[18]   # the sweep raises its thresholds in-launch (csrc/score16.hpp; staged=True switches it off)
	w["ladder_period"] = v[19]   # tiles between two fetches of a wave's ladder counters (LADDER_PERIOD)
	w["gmax_offset"], w["n_groups"] = v[20] * 256, v[21]   # the prepass' group maxima: byte offset in the workspace, row pitch
	w["prepass16"], w["prepass_splits"] = bool(v[22]), v[23]
	return w


def fused_plan(Q, I, Kp, k, leading_sample=False, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""The plan a fused call with these flags runs.  "lg": candidate segments per (query, item split) -- 2 = the 32x32x16 body (per-lane
	rings; the default above k = 1024 -- above 384 under staged=True --, and for Kp = 512), 1 = the 16x16x32 body (one queue per wave; the default for Kp <= 256, k <= 1024),
	4 = the wide kernel (Kp > 512); "QT": 32-query sub-tiles per wave (1 = qt1 honoured, or Kp = 512);
	"stage_pred": body of each sweep stage -- 0 / 1 = 32x32x16 with the ballot / exec-mask filter, 2 = 16x16x32 (4-wave workgroups, barrier per
	tile), 4 = Kp = 512 with the wave queue on 16x16x32.  staged=True (ANNCUR_TOPK_STAGED) switches the ladder off; for Kp <= 256 and k in
	385..1024 it thereby also switches the body from 16x16x32 to 32x32x16 ("lg" 2), not the same body without the ladder.
	ring=True (the retired tile-ring body) raises."""
	out = (ctypes.c_int32 * 20)()
	check(_lib.load().anncur_score_topk_plan_ex(Q, I, Kp, k, _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), out, 20), "score_topk_plan_ex")
	w = _plan_words(out)
	return {key: w[key] for key in _PLAN_HEAD + ("stage_end", "stage_pred", "stage_flush", "ladder", "ladder_top_rank", "ladder_period")}


def eval_fused_plan(Q, I, Kp, k):
	"""The plan eval_fused runs for the cell (host query, no GPU needed): the keys of fused_plan ("stage_pred" 6 = evalf_kernel, no ladder) and
	"stage_tiles_per_split".  Item split s of stage g sweeps the tiles [begin + s * tps, min(begin + (s + 1) * tps, stage_end[g])), begin = the
	previous stage's end: static contiguous shares in item order.  The exact matrix' error terms come from the first I // 32 tiles only."""
	out = (ctypes.c_int32 * 27)()
	check(_lib.load().anncur_eval_fused_plan(Q, I, Kp, k, out, 27), "eval_fused_plan")
	w = _plan_words(out)
	return {key: w[key] for key in _PLAN_HEAD + ("stage_end", "stage_pred", "stage_flush", "stage_tiles_per_split")}


def fused_group_maxima(workspace, Q, I, Kp, k, leading_sample=False, mfma16=False, qt1=False, mfma32=False, ring=False, staged=False):
	"""The prepass output the last score_topk_fused call on `workspace` (same shape and flags) left behind (diagnostics): a float32 view
	[Q x n_groups] into the workspace, gmax[q, 2 j + g] = the maximum score of query q over the 16 rows r of sample tile j with
	(r >> 2) & 1 == g, and {"prepass16": the prepass ran on the sweep's 16x16x32 body, "prepass_splits", "n_groups"}."""
	out = (ctypes.c_int32 * 24)()
	check(_lib.load().anncur_score_topk_plan_ex(Q, I, Kp, k, _topk_flags(leading_sample, mfma16, qt1, mfma32, ring, staged), out, 24), "score_topk_plan_ex")
	w = _plan_words(out)
	off, n_groups = w["gmax_offset"], w["n_groups"]
	gmax = workspace[off:off + Q * n_groups * 4].view(torch.float32).view(Q, n_groups)
	return gmax, {key: w[key] for key in ("prepass16", "prepass_splits", "n_groups")}


def _dense_scores(X, Et):
	"""S = X @ Et^T with fp32 products and sums: the strided fp32-MFMA kernel of this library (any strides, fp32 or bf16 operands).
	No vendor GEMM anywhere on the path."""
	return gemm(X, Et.t())


@_on_device
def score_topk_dense(X, Et, k, max_bytes=2 << 30):
	"""Unfused route: S = X @ Et^T in fp32 (row chunks), then the exact scan.  Any K, any dtype.  bf16 operands of a shape the
	fused kernels take never come here from the index classes (cur.py / nearest_nbr.py try score_topk_fused first); what is left
	are the fp32 route, tiny item sets and tests that want the unfused answer."""
	_dev(X, Et)
	Q, I = X.shape[0], Et.shape[0]
	val = torch.empty((Q, k), dtype=torch.float32, device=X.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=X.device)
	rows = max(1, min(Q, max_bytes // max(4 * I, 1)))
	for q0 in range(0, Q, rows):
		q1 = min(Q, q0 + rows)
		S = _dense_scores(X[q0:q1], Et)
		v, i = rowwise_topk(S, k)
		val[q0:q1], idx[q0:q1] = v, i
	return TopK(val, idx)


# ------------------------------------------------------------------ sparse inner-product search
SPARSE_WINDOW = _lib.SPARSE_WINDOW        # ANNCUR_SPARSE_WINDOW
SPARSE_MAX_QNNZ = _lib.SPARSE_MAX_QNNZ    # ANNCUR_SPARSE_MAX_QNNZ
SPARSE_MAX_Q_PER_CALL = 1 << 20           # queries per library call (the launch is one workgroup per query at least)
_SPARSE_PLAN = ("windows", "windows_per_wave", "spans", "workgroups_per_query", "workgroups", "waves_per_workgroup", "lds_bytes", "pitch", "groups", "max_qnnz")
SparsePostings = namedtuple("SparsePostings", ["term_ptr", "post_item", "post_val", "n_items", "n_terms"])
SparseCSR = namedtuple("SparseCSR", ["indptr", "indices", "data", "n_rows", "n_cols"])


def is_sparse_arg(x):
	"""Is x a CSR operand: an object with .indptr / .indices / .data / .shape (scipy.sparse.csr_matrix is one; scipy is never imported),
	a SparseCSR, or an (indptr, indices, data) triple of 1-D tensors / arrays?"""
	if isinstance(x, SparseCSR) or all(hasattr(x, a) for a in ("indptr", "indices", "data", "shape")):
		return True
	if not (isinstance(x, (tuple, list)) and len(x) == 3 and all(torch.is_tensor(a) or isinstance(a, np.ndarray) for a in x) and all(a.ndim == 1 for a in x)):
		return False
	kinds = ["f" if (a.dtype.is_floating_point if torch.is_tensor(a) else a.dtype.kind == "f") else "i" for a in x]
	return kinds == ["i", "i", "f"]   # (three float rows are a dense matrix)


def _sparse_tensor(a, what, name):
	if torch.is_tensor(a):
		return a.detach()
	a = np.asarray(a)
	if a.dtype == object:
		raise TypeError(f"{what}: {name} is not a numeric array")
	return torch.from_numpy(np.ascontiguousarray(a))


def sparse_csr(x, n_cols=None, what="sparse", max_row_nnz=None):
	"""A CSR operand, checked where it lives (host arrays on the host, before anything touches the device) -> SparseCSR of tensors on that
	same device: indptr int64 [n + 1], indices int32, data fp32.
	x: an (indptr, indices, data) triple -- dtypes must be exactly those, TypeError otherwise; n_cols must be given -- or an object with
	.indptr / .indices / .data / .shape, whose arrays are converted (integer index arrays to int64 / int32, floating data to fp32).
	ValueError: indptr not starting at 0, decreasing or not ending at nnz; a term id outside [0, n_cols) (one reduction); a row whose term
	ids are not strictly ascending -- the first such row is named; the remedy is sort_indices() / sum_duplicates() --; n >= 2^31 - 1,
	n_cols >= 2^31, nnz >= 2^31; max_row_nnz: a row with more stored terms (queries: ANNCUR_SPARSE_MAX_QNNZ)."""
	if isinstance(x, SparseCSR):
		indptr, indices, data, shape, strict = x.indptr, x.indices, x.data, (x.n_rows, x.n_cols), True
	elif isinstance(x, (tuple, list)):
		if len(x) != 3:
			raise ValueError(f"{what}: a CSR operand is an (indptr, indices, data) triple or an object with .indptr / .indices / .data / .shape")
		(indptr, indices, data), shape, strict = x, None, True
	else:
		try:
			indptr, indices, data, shape, strict = x.indptr, x.indices, x.data, tuple(int(s) for s in x.shape), False
		except AttributeError:
			raise TypeError(f"{what}: expected a CSR operand (an (indptr, indices, data) triple or an object with .indptr / .indices / .data / .shape), "
							f"got {type(x).__name__}") from None
		fmt = getattr(x, "format", "csr")
		if fmt != "csr":
			raise TypeError(f"{what}: the sparse matrix is in {fmt} format, CSR is required (tocsr())")
	indptr, indices, data = (_sparse_tensor(a, what, n) for a, n in ((indptr, "indptr"), (indices, "indices"), (data, "data")))
	if not strict:
		for a, n in ((indptr, "indptr"), (indices, "indices")):
			if a.dtype not in (torch.int32, torch.int64):
				raise TypeError(f"{what}: {n} must be an int32 or int64 array (got {a.dtype})")
		if not data.dtype.is_floating_point:
			raise TypeError(f"{what}: data must be a floating-point array (got {data.dtype})")
		indptr, data = indptr.to(torch.int64), data.to(torch.float32)
	if indptr.dtype != torch.int64 or indices.dtype not in (torch.int32, torch.int64) or (strict and indices.dtype != torch.int32) or data.dtype != torch.float32:
		raise TypeError(f"{what}: a CSR triple is (indptr int64, indices int32, data float32), got ({indptr.dtype}, {indices.dtype}, {data.dtype})")
	if indptr.dim() != 1 or indices.dim() != 1 or data.dim() != 1 or indptr.numel() < 1:
		raise ValueError(f"{what}: indptr [n + 1], indices [nnz] and data [nnz] must be 1-D arrays")
	n, nnz = indptr.numel() - 1, indices.numel()
	if shape is not None:
		if len(shape) != 2 or shape[0] != n:
			raise ValueError(f"{what}: shape {tuple(shape)} does not go with an indptr of {n + 1} entries")
		if n_cols is not None and shape[1] != n_cols:
			raise ValueError(f"{what}: the matrix has {shape[1]} columns, expected {n_cols}")
		n_cols = shape[1]
	if n_cols is None:
		raise ValueError(f"{what}: the number of columns (terms) of a CSR triple must be given")
	n_cols = int(n_cols)
	if data.numel() != nnz:
		raise ValueError(f"{what}: indices holds {nnz} entries, data {data.numel()}")
	if n >= (1 << 31) - 1:
		raise ValueError(f"{what}: n = {n} rows, the limit is n < 2^31 - 1")
	if not 0 <= n_cols < (1 << 31):
		raise ValueError(f"{what}: V = {n_cols} terms, the limit is V < 2^31")
	if nnz >= (1 << 31):
		raise ValueError(f"{what}: nnz = {nnz} stored entries, the limit is nnz < 2^31")
	first, last = int(indptr[0]), int(indptr[-1])
	if first != 0 or last != nnz:
		raise ValueError(f"{what}: indptr must start at 0 and end at nnz = {nnz} (got indptr[0] = {first}, indptr[-1] = {last})")
	counts = indptr[1:] - indptr[:-1]
	if n and int(counts.min()) < 0:
		raise ValueError(f"{what}: indptr decreases at row {int(torch.nonzero(counts < 0)[0])}")
	if nnz:
		lo, hi = (int(v) for v in torch.aminmax(indices))
		if lo < 0 or hi >= n_cols:
			raise ValueError(f"{what}: term id {lo if lo < 0 else hi} is outside [0, {n_cols})")
	if indices.dtype != torch.int32:
		indices = indices.to(torch.int32)
	if nnz > 1:
		ok = indices[1:] > indices[:-1]
		starts = indptr[1:-1]
		ok[starts[(starts > 0) & (starts < nnz)] - 1] = True      # the first entry of a row has no predecessor in its row
		if not bool(ok.all()):
			p = int(torch.nonzero(~ok)[0]) + 1
			row = int(torch.searchsorted(indptr, torch.tensor([p], dtype=torch.int64, device=indptr.device), right=True)[0]) - 1
			a, b = int(indices[p - 1]), int(indices[p])
			raise ValueError(f"{what}: row {row} is not in canonical form: " + (f"duplicate term {b}" if a == b else f"unsorted, term {b} follows term {a}")
							 + "; the term ids of a row must be strictly ascending (scipy: sort_indices() / sum_duplicates())")
	if max_row_nnz is not None and n and int(counts.max()) > max_row_nnz:
		row = int(torch.nonzero(counts > max_row_nnz)[0])
		raise ValueError(f"{what}: row {row} stores {int(counts[row])} terms, above ANNCUR_SPARSE_MAX_QNNZ = {max_row_nnz} stored terms per query")
	return SparseCSR(indptr.contiguous(), indices.contiguous(), data.contiguous(), n, n_cols)


def sparse_from_dense(M):
	"""Dense [n x V] floating array / tensor -> SparseCSR of its non-zero entries (row-major order is canonical form), on M's device."""
	M = torch.as_tensor(np.ascontiguousarray(M, dtype=np.float32)) if not torch.is_tensor(M) else M.detach().to(torch.float32)
	if M.dim() != 2:
		raise ValueError("sparse_from_dense: expected a 2-D array")
	nz = M != 0
	indptr = torch.zeros(M.shape[0] + 1, dtype=torch.int64, device=M.device)
	indptr[1:] = torch.cumsum(nz.sum(dim=1), dim=0)
	rc = torch.nonzero(nz)
	return SparseCSR(indptr, rc[:, 1].to(torch.int32).contiguous(), M[nz].contiguous(), M.shape[0], M.shape[1])


def _sparse_k_check(what, k, n):
	limit = min(n, _lib.MAX_TOPK)
	if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= limit:
		raise ValueError(f"{what}: k = {k} outside 1..min(n, ANNCUR_MAX_TOPK) = min({n}, {_lib.MAX_TOPK}) = {limit}")


def sparse_postings(indptr, indices, data, n_items, n_terms, device=None):
	"""The term-major (inverted) index of a CSR item matrix [n_items x n_terms] on the device: term_ptr int64 [V + 1], post_item int32 [nnz]
	(ascending inside a term), post_val fp32 [nnz].  Canonical form and the limits are checked first (sparse_csr), where the arrays live.
	The transposition is torch's stable sort by term id + bincount + cumsum on the device."""
	csr = sparse_csr((indptr, indices, data), n_terms, "sparse_postings")
	if csr.n_rows != n_items:
		raise ValueError(f"sparse_postings: indptr has {csr.n_rows + 1} entries, expected n_items + 1 = {n_items + 1}")
	if n_items < 1:
		raise ValueError("sparse_postings: the index needs at least one item")
	return _postings_of(csr, device)


def _postings_of(csr, device=None):
	if device is None:
		device = csr.indptr.device if csr.indptr.is_cuda else torch.device("cuda", torch.cuda.current_device())
	device = torch.device(device)
	indptr, indices, data = (a.to(device) for a in csr[:3])
	with torch.cuda.device(device):
		counts = indptr[1:] - indptr[:-1]
		rows = torch.repeat_interleave(torch.arange(csr.n_rows, dtype=torch.int32, device=device), counts)
		order = torch.sort(indices, stable=True).indices
		term_ptr = torch.zeros(csr.n_cols + 1, dtype=torch.int64, device=device)
		if indices.numel():
			term_ptr[1:] = torch.cumsum(torch.bincount(indices, minlength=csr.n_cols), dim=0)
		return SparsePostings(term_ptr, rows[order].contiguous(), data[order].contiguous(), csr.n_rows, csr.n_cols)


def _sparse_queries(what, queries, postings):
	if not isinstance(postings, SparsePostings):
		raise TypeError(f"{what}: postings must come from sparse_postings()")
	return sparse_csr(queries, postings.n_terms, what, max_row_nnz=SPARSE_MAX_QNNZ)   # (an object's own .shape[1] must equal the index' terms)


def sparse_plan(Q, I):
	"""The plan of a sparse scoring launch (host query): windows of SPARSE_WINDOW items per query, windows per wave, spans (waves with work)
	and workgroups per query, workgroups, waves per workgroup, LDS bytes per workgroup, the pitch of the score scratch in floats, groups of
	64 items, ANNCUR_SPARSE_MAX_QNNZ."""
	if not 1 <= Q or not 1 <= I < (1 << 31) - 1:
		raise ValueError(f"sparse_plan: (Q = {Q}, I = {I}) is outside Q >= 1, 1 <= I < 2^31 - 1")
	out = (ctypes.c_int32 * len(_SPARSE_PLAN))()
	check(_lib.load().anncur_sparse_plan(Q, I, out, len(_SPARSE_PLAN)), "sparse_plan")
	w = dict(zip(_SPARSE_PLAN, (int(x) for x in out)))
	w["pitch"] *= 32
	return w


def sparse_workspace(Q, I, k, device):
	"""A private workspace for sparse_score_topk (256-byte aligned uint8 tensor) that holds the score rows of Q queries."""
	nbytes = _lib.load().anncur_sparse_score_topk_workspace_bytes(Q, I, k)
	buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
	off = (-buf.data_ptr()) % 256
	return buf[off:off + nbytes]


def _sparse_args(csr, postings, q0, q1):
	ip = csr.indptr[q0:q1 + 1]
	return (_p(ip), _p(csr.indices) if csr.indices.numel() else None, _p(csr.data) if csr.data.numel() else None, q1 - q0, _p(postings.term_ptr),
			_p(postings.post_item) if postings.post_item.numel() else None, _p(postings.post_val) if postings.post_val.numel() else None,
			postings.n_terms, postings.n_items)


def sparse_score_rows(queries, postings):
	"""The scoring launch alone, for audits on small shapes -> (S [Q x I] fp32, a view of rows ceil32(I) apart, GM [Q x ceil(I / 64)] fp32:
	the maximum of every 64 consecutive items).  S[q, i] is the ascending-term fp32 chain of include/anncur_hip.h."""
	csr = _sparse_queries("sparse_score_rows", queries, postings)
	dev = postings.term_ptr.device
	_dev(postings.term_ptr, postings.post_item, postings.post_val)
	csr = SparseCSR(*(a.to(dev) for a in csr[:3]), csr.n_rows, csr.n_cols)
	Q, I = csr.n_rows, postings.n_items
	pitch, G = -(-I // 32) * 32, -(-I // 64)
	with torch.cuda.device(dev):
		S = torch.empty((Q, pitch), dtype=torch.float32, device=dev)
		GM = torch.empty((Q, G), dtype=torch.float32, device=dev)
		for q0 in range(0, Q, SPARSE_MAX_Q_PER_CALL):
			q1 = min(Q, q0 + SPARSE_MAX_Q_PER_CALL)
			check(_lib.load().anncur_sparse_score_rows(*_sparse_args(csr, postings, q0, q1), _p(S[q0:q1]), pitch, _p(GM[q0:q1]), G, _stream()), "sparse_score_rows")
	return S[:, :I], GM


def sparse_score_topk(queries, postings, k, exclude=None, max_bytes=2 << 30, workspace=None):
	"""Exact top-k of the sparse inner products: queries (a CSR object or triple, on the host or the device) against sparse_postings() ->
	TopK(values f32 [Q x k], indices int32 [Q x k]), score descending, equal scores to the smaller item id, (-inf, -1) pads.  The score rows
	of a chunk of queries go into the workspace (at most max_bytes, at least one query), then the exact scan.  exclude: as every other
	route, k + the longest list candidates per query, then filter_topk.  workspace: a 256-byte aligned uint8 tensor for one chunk
	(sparse_workspace); default = the grow-only buffer of the fused route."""
	csr = _sparse_queries("sparse_score_topk", queries, postings)
	Q, I = csr.n_rows, postings.n_items
	_sparse_k_check("sparse_score_topk", k, I)
	dev = postings.term_ptr.device
	excl, kc = None, int(k)
	if exclude is not None:
		excl = exclusion(exclude, Q, I, dev)
		if excl.e_max == 0:
			excl = None
		else:
			kc = filtered_k(int(k), excl.e_max, I)
	_dev(postings.term_ptr, postings.post_item, postings.post_val)
	csr = SparseCSR(*(a.to(dev) for a in csr[:3]), csr.n_rows, csr.n_cols)
	lib = _lib.load()
	pitch = -(-I // 32) * 32
	rows = max(1, min(Q, max_bytes // (4 * pitch), SPARSE_MAX_Q_PER_CALL))
	with torch.cuda.device(dev):
		val = torch.empty((Q, kc), dtype=torch.float32, device=dev)
		idx = torch.empty((Q, kc), dtype=torch.int32, device=dev)
		if Q:
			nbytes = lib.anncur_sparse_score_topk_workspace_bytes(rows, I, kc)
			if workspace is None:
				ws = _Workspace.get(nbytes, dev)
			else:
				ws = workspace
				if ws.numel() < nbytes or ws.data_ptr() % 256 != 0 or ws.device != dev:
					raise ValueError(f"sparse_score_topk: workspace too small ({ws.numel()} of {nbytes} bytes), misaligned or on another device (use sparse_workspace())")
		for q0 in range(0, Q, rows):
			q1 = min(Q, q0 + rows)
			check(lib.anncur_sparse_score_topk(*_sparse_args(csr, postings, q0, q1), kc, _p(val[q0:q1]), _p(idx[q0:q1]), _p(ws), ws.numel(), _stream()),
				  "sparse_score_topk")
		if excl is not None:
			return filter_topk(val, idx, excl, int(k))
	return TopK(val, idx)


# ------------------------------------------------------------------ ranks of given items
RANK_MAX_T = _lib.RANK_MAX_T
_RANK_KP = (64, 128, 256, 512)


def _rank_ids(ids, Q, I, what):
	"""The target ids of a rank call, checked on the host before anything touches the device: int32 [Q x t] (tensor on any device, or a NumPy
	array), 1 <= t <= RANK_MAX_T, every id in [0, I) or -1 (a hole).  A wrong dtype is a TypeError, everything else a ValueError.  Ids that live
	on the GPU cost one synchronisation for their minimum and maximum: an id outside the row is never a device read."""
	if not torch.is_tensor(ids):
		ids = torch.as_tensor(np.asarray(ids))
	if ids.dtype != torch.int32:
		raise TypeError(f"{what}: ids must be int32 (got {ids.dtype})")
	if ids.dim() != 2 or ids.shape[0] != Q:
		raise ValueError(f"{what}: ids must be [Q x t] with Q = {Q} rows (got {tuple(ids.shape)})")
	t = ids.shape[1]
	if not 1 <= t <= RANK_MAX_T:
		raise ValueError(f"{what}: t = {t} targets per row, need 1 <= t <= {RANK_MAX_T}")
	if ids.numel():
		lo, hi = (int(v) for v in torch.aminmax(ids))
		if lo < -1 or hi >= I:
			raise ValueError(f"{what}: id {lo if lo < -1 else hi} is outside [0, {I}) and is not the hole -1")
	return ids


def _rank_out(Q, t, device, return_scores):
	rank = torch.empty((Q, t), dtype=torch.int32, device=device)
	score = torch.empty((Q, t), dtype=torch.float32, device=device) if return_scores else None
	return rank, score


@_on_device
def rank_in_rows(S, ids, return_scores=False):
	"""rank[q, j] = the position of item ids[q, j] in row q of S sorted by score descending, ties to the smaller id (the order of
	rowwise_topk): #{i != id : S[q, i] > a or (S[q, i] == a and i < id)}, a = S[q, id].  -0.0 ties with +0.0, a NaN is never ahead of
	anything, a NaN target and a hole (id -1) get rank -1; duplicate ids are allowed.  S [Q x I] fp32 / bf16 (rows may be padded), ids int32
	[Q x t], 1 <= t <= RANK_MAX_T.  -> rank int32 [Q x t], with return_scores (rank, score fp32 [Q x t]): the targets' scores (NaN for a hole)."""
	if not torch.is_tensor(S) or S.dim() != 2:
		raise ValueError("rank_in_rows: S must be a 2-D tensor")
	dt = _dt(S)
	Q, I = S.shape
	if I < 1:
		raise ValueError("rank_in_rows: S has no columns")
	ids = _rank_ids(ids, Q, I, "rank_in_rows")
	_dev(S)
	S = _rowmajor(S)
	ids = ids.to(S.device).contiguous()
	rank, score = _rank_out(Q, ids.shape[1], S.device, return_scores)
	check(_lib.load().anncur_rank_in_rows(_p(S), dt, Q, I, _ld(S), _p(ids), ids.shape[1], _p(rank), _p(score) if return_scores else None, _stream()), "rank_in_rows")
	return (rank, score) if return_scores else rank


def score_rank_ok(Kp, I, t):
	"""True if anncur_score_rank takes this shape: the packed widths of approx_error_packed, at most RANK_MAX_T targets per query."""
	return Kp in _RANK_KP and 1 <= t <= RANK_MAX_T and 1 <= I < (1 << 31) - 65


@_on_device
def score_rank(Xp, Etp, I, ids, return_scores=False, workspace=None):
	"""rank_in_rows under S_hat = Xp . Etp^T without writing S_hat: Xp [Q x Kp] packed bf16, Etp [ceil32(I) x Kp] packed bf16 in ITEM order
	(pack_bf16(..., row_multiple=32); a descending-norm copy is NOT item order), Kp in {64, 128, 256, 512}.  A target's score is computed by
	the counting pass' own tile routine, so it is bit-identical to the score that pass compares it with.  workspace: a private 256-byte
	aligned uint8 tensor of anncur_score_rank_workspace_bytes (default: the shared grow-only one); nothing in it needs to be pre-filled."""
	for name, M in (("Xp", Xp), ("Etp", Etp)):
		if not torch.is_tensor(M) or M.dim() != 2:
			raise ValueError(f"score_rank: {name} must be a 2-D tensor")
		if M.dtype != torch.bfloat16:
			raise TypeError(f"score_rank: {name} must be packed bfloat16 (got {M.dtype})")
	Q, Kp = Xp.shape
	if Kp not in _RANK_KP or Etp.shape[1] != Kp or I < 1 or Etp.shape[0] < -(-I // 32) * 32:
		raise ValueError(f"score_rank: Xp [Q x Kp], Etp [ceil32(I) x Kp] with Kp in {_RANK_KP} (got Xp {tuple(Xp.shape)}, Etp {tuple(Etp.shape)}, I = {I})")
	ids = _rank_ids(ids, Q, I, "score_rank")
	if not score_rank_ok(Kp, I, ids.shape[1]):
		raise ValueError(f"score_rank: shape (I = {I}, Kp = {Kp}, t = {ids.shape[1]}) is outside the fused route")
	_dev(Xp, Etp)
	if not Etp.is_contiguous():
		raise ValueError("score_rank: Etp must be contiguous")
	Xp = _rowmajor(Xp)
	if _ld(Xp) % 8 != 0 or Xp.data_ptr() % 16 != 0:
		Xp = Xp.contiguous()
	ids = ids.to(Xp.device).contiguous()
	t = ids.shape[1]
	rank, score = _rank_out(Q, t, Xp.device, return_scores)
	if Q == 0:
		return (rank, score) if return_scores else rank
	lib = _lib.load()
	nbytes = lib.anncur_score_rank_workspace_bytes(Q, I, Kp, t)
	if nbytes == 0:
		raise _lib.AnncurHipError(f"score_rank: shape (Q={Q}, I={I}, Kp={Kp}, t={t}) is outside the fused route")
	if workspace is None:
		workspace = _Workspace.get(nbytes, Xp.device)
	elif workspace.dtype != torch.uint8 or workspace.numel() < nbytes or workspace.data_ptr() % 256 != 0 or not workspace.is_contiguous():
		raise ValueError(f"score_rank: workspace must be a contiguous 256-byte aligned uint8 tensor of at least {nbytes} bytes")
	check(lib.anncur_score_rank(_p(Xp), _ld(Xp), _p(Etp), Kp, Q, I, Kp, _p(ids), t, _p(rank), _p(score) if return_scores else None,
								_p(workspace), workspace.numel(), _stream()), "score_rank")
	return (rank, score) if return_scores else rank


@_on_device
def rank_dense(X, Et, ids, max_bytes=2 << 30, return_scores=False):
	"""Unfused route of the ranks: S = X @ Et^T in fp32 in row chunks of at most max_bytes, exactly as score_topk_dense takes it, and
	rank_in_rows on each chunk.  Any K, any dtype: the scores are the ones score_topk_dense ranks."""
	if not torch.is_tensor(X) or not torch.is_tensor(Et) or X.dim() != 2 or Et.dim() != 2 or X.shape[1] != Et.shape[1]:
		raise ValueError("rank_dense: X [Q x K] and Et [I x K] must be 2-D tensors with one inner dimension")
	_dt(X), _dt(Et)
	Q, I = X.shape[0], Et.shape[0]
	ids = _rank_ids(ids, Q, I, "rank_dense")
	_dev(X, Et)
	ids = ids.to(X.device).contiguous()
	rank, score = _rank_out(Q, ids.shape[1], X.device, return_scores)
	rows = max(1, min(Q, max_bytes // max(4 * I, 1)))
	for q0 in range(0, Q, rows):
		q1 = min(Q, q0 + rows)
		res = rank_in_rows(_dense_scores(X[q0:q1], Et), ids[q0:q1], return_scores)
		if return_scores:
			rank[q0:q1], score[q0:q1] = res
		else:
			rank[q0:q1] = res
	return (rank, score) if return_scores else rank


# ------------------------------------------------------------------ SoftMax item sampling
def _temperature_arg(temperature, what):
	if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)) or not np.isfinite(temperature) or not temperature > 0:
		raise ValueError(f"{what}: temperature = {temperature!r}, need a finite temperature > 0")
	return float(temperature)


def _noise_args(seed, stream, what):
	"""(seed, stream) as Python ints inside the counter's fields, or a ValueError that names the limit."""
	for name, v, bits in (("seed", seed, 64), ("stream", stream, 32)):
		if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
			raise ValueError(f"{what}: {name} must be an integer in [0, 2^{bits}) (got {v!r})")
		if not 0 <= int(v) < (1 << bits):
			raise ValueError(f"{what}: {name} = {int(v)} outside [0, 2^{bits})")
	return int(seed), int(stream)


def _row_keys(row_keys, Q, device, what):
	"""row_keys= -> None (the row numbers) or int32 [Q] on `device` holding the low 32 bits of every key (the kernels read them as uint32)."""
	if row_keys is None:
		return None
	t = row_keys if torch.is_tensor(row_keys) else torch.as_tensor(np.asarray(row_keys))
	if t.dim() != 1 or t.numel() != Q:
		raise ValueError(f"{what}: row_keys must hold one key per row: {Q} (got shape {tuple(t.shape)})")
	if t.dtype.is_floating_point or t.dtype == torch.bool:
		raise ValueError(f"{what}: row_keys must be integers (got {t.dtype})")
	t = t.to(torch.int64)
	return ((((t & 0xffffffff) ^ 0x80000000) - 0x80000000).to(torch.int32)).to(device).contiguous()   # low 32 bits, as the int32 of the same bit pattern


def _sample_args(Q, I, k, temperature, seed, stream, row_keys):
	"""Host-side validation of sample_topk, before any tensor has to be on the GPU: -> (inv_T as numpy.float32, seed, stream)."""
	with np.errstate(over="ignore", under="ignore"):
		inv_T = np.float32(1.0 / _temperature_arg(temperature, "sample_topk"))
	if not (np.isfinite(inv_T) and inv_T > 0):
		raise ValueError(f"sample_topk: temperature = {temperature!r}: 1 / temperature = {inv_T} is not a finite fp32 number > 0")
	seed, stream = _noise_args(seed, stream, "sample_topk")
	if I >= 1 << 31:
		raise ValueError(f"sample_topk: {I} items, need fewer than 2^31")
	limit = min(I, _lib.MAX_TOPK)
	if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > limit:
		raise ValueError(f"sample_topk: k = {k!r} outside 1..min(items, ANNCUR_MAX_TOPK) = min({I}, {_lib.MAX_TOPK}) = {limit}")
	if row_keys is not None:
		n = row_keys.numel() if torch.is_tensor(row_keys) else np.asarray(row_keys).size
		if n != Q:
			raise ValueError(f"sample_topk: row_keys must hold one key per row: {Q} (got {n})")
	return inv_T, seed, stream


@_on_device
def gumbel_noise(seed, stream, rows, I):
	"""g [Q x I] fp32: the standard Gumbel noise the sampler adds to row key r, item i (anncur_gumbel_noise; the contract is in
	include/anncur_hip.h).  rows: an int (the keys 0..rows-1) or a 1-D integer tensor / array of keys (their low 32 bits count).  For tests
	and for auditing a draw: sample_topk never materialises it.  On the device of `rows` if that is a GPU tensor, else on the current one."""
	seed, stream = _noise_args(seed, stream, "gumbel_noise")
	if isinstance(rows, (int, np.integer)) and not isinstance(rows, bool):
		Q, keys = int(rows), None
		if Q < 0:
			raise ValueError(f"gumbel_noise: rows = {Q}, need rows >= 0")
	else:
		Q, keys = (rows.numel() if torch.is_tensor(rows) else np.asarray(rows).size), rows
	if not 1 <= I <= 1 << 31:
		raise ValueError(f"gumbel_noise: I = {I} outside 1..2^31 (item ids are 31-bit)")
	device = rows.device if torch.is_tensor(rows) and rows.is_cuda else torch.device("cuda", torch.cuda.current_device())
	keys = _row_keys(keys, Q, device, "gumbel_noise")
	with torch.cuda.device(device):
		out = torch.empty((Q, I), dtype=torch.float32, device=device)
		check(_lib.load().anncur_gumbel_noise(seed, stream, _p(keys) if keys is not None else None, Q, I, _p(out), I, _stream()), "gumbel_noise")
	return out


@_on_device
def sample_topk(S, k, temperature=1.0, seed=0, stream=0, row_keys=None, exclude=None):
	"""k items per row of S (fp32 [Q x I], rows may be padded) drawn WITHOUT replacement with probability proportional to
	softmax(S / temperature): Gumbel top-k (anncur_sample_topk) -> TopK(keys f32 [Q x k], indices int32 [Q x k]), the perturbed keys
	S / temperature + g descending, ties by the smaller id, (-inf, -1) where a row has fewer than k allowed non-NaN items.  The noise g is a
	pure function of (seed, stream, row key, item id): row_keys (one integer per row, low 32 bits; default the row numbers) name the rows, so
	a row draws the same items wherever it stands in a call.  exclude: anything exclusion() takes; an Exclusion passes through.
	ValueError (before any device call): temperature not finite or <= 0, seed outside [0, 2^64), stream outside [0, 2^32), k outside
	1..min(I, ANNCUR_MAX_TOPK), row_keys of the wrong length."""
	if not torch.is_tensor(S) or S.dim() != 2:
		raise ValueError("sample_topk: S must be a 2-D tensor [Q x I]")
	Q, I = S.shape
	inv_T, seed, stream = _sample_args(Q, I, k, temperature, seed, stream, row_keys)
	_dev(S)
	if S.dtype != torch.float32:
		raise TypeError(f"sample_topk takes float32 scores (got {S.dtype})")
	S = _rowmajor(S)
	keys = _row_keys(row_keys, Q, S.device, "sample_topk")
	ex = exclusion(exclude, Q, I, S.device)
	n_ids = ex.ids.numel() if ex.ids is not None else 0
	val = torch.empty((Q, k), dtype=torch.float32, device=S.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=S.device)
	check(_lib.load().anncur_sample_topk(_p(S), _ld(S), Q, I, float(inv_T), seed, stream, _p(keys) if keys is not None else None,
										 _p(ex.off) if ex.off is not None else None, _p(ex.ids) if n_ids else None, n_ids if ex.off is None else 0, int(k),
										 _p(val), _p(idx), _stream()), "sample_topk")
	return TopK(val, idx)


@_on_device
def sample_topk_dense(X, Et, k, temperature=1.0, seed=0, stream=0, row_keys=None, exclude=None, max_bytes=2 << 30):
	"""sample_topk on S = X @ Et^T without holding S: score_topk_dense's loop over row chunks -- the fp32 GEMM of a chunk, then the sampler
	on it, with the chunk's row keys and the chunk's slice of the exclusion's offsets (they are absolute: a view suffices).  The noise
	belongs to (row key, item), so the result does not depend on max_bytes."""
	Q, I = X.shape[0], Et.shape[0]
	_sample_args(Q, I, k, temperature, seed, stream, row_keys)
	_dev(X, Et)
	keys = _row_keys(row_keys, Q, X.device, "sample_topk_dense")
	if keys is None:
		keys = torch.arange(Q, dtype=torch.int32, device=X.device)   # (a chunk's row numbers start at 0: name the rows explicitly)
	ex = exclusion(exclude, Q, I, X.device)
	val = torch.empty((Q, k), dtype=torch.float32, device=X.device)
	idx = torch.empty((Q, k), dtype=torch.int32, device=X.device)
	rows = max(1, min(Q, max_bytes // max(4 * I, 1)))
	for q0 in range(0, Q, rows):
		q1 = min(Q, q0 + rows)
		S = _dense_scores(X[q0:q1], Et)
		ex_c = ex if ex.off is None else Exclusion(ex.off[q0:q1 + 1], ex.ids, ex.e_max)
		v, i = sample_topk(S, k, temperature, seed, stream, keys[q0:q1], ex_c)
		val[q0:q1], idx[q0:q1] = v, i
	return TopK(val, idx)


@_on_device
def rerank(A, approx_idx, k_retvr, k_out):
	"""The k_out best of approx_idx[:, :k_retvr] by exact score A (reference: ..._splits.py:93-96)."""
	_dev(A, approx_idx)
	A = _rowmajor(A)
	if approx_idx.dtype != torch.int32 or approx_idx.stride(1) != 1:
		approx_idx = approx_idx.to(torch.int32).contiguous()
	Q, I = A.shape
	val = torch.empty((Q, k_out), dtype=torch.float32, device=A.device)
	idx = torch.empty((Q, k_out), dtype=torch.int32, device=A.device)
	check(_lib.load().anncur_rerank(_p(A), _dt(A), Q, I, _ld(A), _p(approx_idx), _ld(approx_idx), k_retvr, k_out, _p(val), _p(idx),
									_stream()), "rerank")
	return TopK(val, idx)


# ------------------------------------------------------------------ re-rank from caller-supplied scores
SharedIds = namedtuple("SharedIds", ["ids", "n"])
MAX_SHARED_IDS = 65535   # n_sh limit of anncur_rerank_scored


def shared_id_list(ids, device):
	"""The `shared_ids=` argument of rerank_scored -> SharedIds(ids int32 on `device`, n), checked on the host: a flat list of
	non-negative int32 ids, STRICTLY ASCENDING (nothing is sorted here: column j of shared_scores belongs to ids[j], and the kernel
	binary-searches the list).  ValueError otherwise.  A SharedIds passes through, so a searcher checks its anchor ids once; a list
	given as a GPU tensor is copied to the host here, a synchronisation (the rule of exclusion())."""
	if isinstance(ids, SharedIds):
		return ids
	a = np.asarray(_host_array(ids))
	if a.ndim != 1:
		raise ValueError("rerank_scored: shared_ids must be a flat list of item ids")
	if a.size and not np.issubdtype(a.dtype, np.integer):
		raise ValueError("rerank_scored: shared_ids must hold integer item ids")
	a = a.astype(np.int64)
	if a.size > MAX_SHARED_IDS:
		raise ValueError(f"rerank_scored: {a.size} shared ids, above the limit of {MAX_SHARED_IDS}")
	if a.size:
		if int(a[0]) < 0:
			raise ValueError(f"rerank_scored: shared_ids holds the negative id {int(a[0])}")
		if int(a.max()) > 0x7fffffff:
			raise ValueError(f"rerank_scored: shared_ids holds the id {int(a.max())}, beyond int32")
		bad = np.flatnonzero(a[1:] <= a[:-1])
		if bad.size:
			j = int(bad[0])
			raise ValueError(f"rerank_scored: shared_ids must be strictly ascending (ids[{j}] = {int(a[j])}, ids[{j + 1}] = {int(a[j + 1])}); "
							 "sort the ids and the columns of shared_scores together")
	return SharedIds(torch.from_numpy(a.astype(np.int32)).to(device), int(a.size))


def _rerank_scored_args(k, cand, cand_scores, shared_ids, shared_scores):
	"""Host-side validation of rerank_scored, before any tensor has to be on the GPU: -> (Q, n_sh, n_pq, cand indices or None)."""
	if isinstance(cand, TopK):
		cand = cand.indices
	if (cand is None) != (cand_scores is None):
		raise ValueError("rerank_scored: cand and cand_scores come together")
	if (shared_ids is None) != (shared_scores is None):
		raise ValueError("rerank_scored: shared_ids and shared_scores come together")
	Q = None
	n_pq = n_sh = 0
	if cand is not None:
		if not (torch.is_tensor(cand) and torch.is_tensor(cand_scores)) or cand.dim() != 2 or tuple(cand.shape) != tuple(cand_scores.shape):
			raise ValueError("rerank_scored: cand and cand_scores must be 2-D tensors [Q x n_pq] of one shape")
		if cand.dtype != torch.int32:
			raise ValueError(f"rerank_scored: cand must hold int32 ids (got {cand.dtype})")
		if cand_scores.dtype != torch.float32:
			raise ValueError(f"rerank_scored: cand_scores must be float32 (got {cand_scores.dtype})")
		Q, n_pq = cand.shape
		if n_pq > _lib.MAX_TOPK:
			raise ValueError(f"rerank_scored: {n_pq} candidates per query, above the limit of ANNCUR_MAX_TOPK = {_lib.MAX_TOPK}")
	if shared_ids is not None:
		n_sh = shared_ids.n if isinstance(shared_ids, SharedIds) else len(shared_ids)
		if not torch.is_tensor(shared_scores) or shared_scores.dim() != 2 or shared_scores.shape[1] != n_sh:
			raise ValueError(f"rerank_scored: shared_scores must be a 2-D tensor [Q x {n_sh}], one column per shared id")
		if shared_scores.dtype not in _DT:
			raise ValueError(f"rerank_scored: shared_scores must be float32 or bfloat16 (got {shared_scores.dtype})")
		if n_sh > MAX_SHARED_IDS:
			raise ValueError(f"rerank_scored: {n_sh} shared ids, above the limit of {MAX_SHARED_IDS}")
		if Q is not None and shared_scores.shape[0] != Q:
			raise ValueError(f"rerank_scored: shared_scores has {shared_scores.shape[0]} rows, cand has {Q}")
		Q = shared_scores.shape[0]
	if n_sh + n_pq < 1:
		raise ValueError("rerank_scored: the pool is empty: give cand / cand_scores, shared_ids / shared_scores or both")
	limit = min(n_sh + n_pq, _lib.MAX_TOPK)
	if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > limit:
		raise ValueError(f"rerank_scored: k = {k} outside 1..min(pool size, ANNCUR_MAX_TOPK) = min({n_sh + n_pq}, {_lib.MAX_TOPK}) = {limit}")
	return Q, n_sh, n_pq, cand


@_on_device
def rerank_scored(k, cand=None, cand_scores=None, shared_ids=None, shared_scores=None):
	"""The k best of a pool of items whose exact scores the CALLER holds (reference: ..._splits.py:91-96 without the resident matrix):
	  cand [Q x n_pq] int32 ids (or a TopK: its .indices; id < 0 = hole) with cand_scores [Q x n_pq] float32, in candidate order;
	  shared_ids [n_sh] strictly ascending, one list for all queries, with shared_scores [Q x n_sh] float32 / bfloat16 -- the anchor scores X.
	Either source may be missing.  A candidate that is also a shared id is dropped (the shared score stands).  -> TopK, score descending,
	ties by the smaller id, NaN never selected, (-inf, -1) padding.  Validated on the host (ValueError with the limit); nothing is sorted."""
	Q, n_sh, n_pq, cand = _rerank_scored_args(k, cand, cand_scores, shared_ids, shared_scores)
	dev = (shared_scores if cand is None else cand).device
	sh = None
	if shared_ids is not None:
		sh = shared_id_list(shared_ids, dev)
		_dev(shared_scores, sh.ids)
		shared_scores = _rowmajor(shared_scores)
	if cand is not None:
		_dev(cand, cand_scores)
		cand, cand_scores = _rowmajor(cand), _rowmajor(cand_scores)
		if _ld(cand) != _ld(cand_scores):
			cand, cand_scores = cand.contiguous(), cand_scores.contiguous()
	val = torch.empty((Q, k), dtype=torch.float32, device=dev)
	idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
	check(_lib.load().anncur_rerank_scored(_p(sh.ids) if n_sh else None, _p(shared_scores) if n_sh else None, _dt(shared_scores) if n_sh else F32,
										   _ld(shared_scores) if n_sh else 0, n_sh, _p(cand) if n_pq else None, _p(cand_scores) if n_pq else None,
										   _ld(cand) if n_pq else 0, n_pq, Q, int(k), _p(val), _p(idx), _stream()), "rerank_scored")
	return TopK(val, idx)


# ------------------------------------------------------------------ adaptive multi-round search
LSTSQ_WS_LIMIT_BYTES = 2 << 30   # default cap of lstsq_rows' workspace: more queries than fit run in chunks


def _lstsq_check(Q, n, kq, ridge):
	"""The limits of anncur_lstsq_rows, as ValueErrors that name them (nothing needs a GPU here)."""
	if n < 1 or n > _lib.MAX_TOPK:
		raise ValueError(f"lstsq_rows: {n} scored items per query, outside 1..ANNCUR_MAX_TOPK = {_lib.MAX_TOPK}")
	if kq < 1 or kq > _lib.LSTSQ_MAX_KQ:
		raise ValueError(f"lstsq_rows: kq = {kq} anchor queries, outside 1..ANNCUR_LSTSQ_MAX_KQ = {_lib.LSTSQ_MAX_KQ}")
	if min(n, kq) > _lib.LSTSQ_MAX_G:
		raise ValueError(f"lstsq_rows: g = min(n, kq) = min({n}, {kq}) = {min(n, kq)}, above ANNCUR_LSTSQ_MAX_G = {_lib.LSTSQ_MAX_G}")
	if not ridge >= 0.0:
		raise ValueError(f"lstsq_rows: ridge = {ridge}, need ridge >= 0")


def lstsq_workspace_bytes(Q, n, kq):
	return _lib.load().anncur_lstsq_rows_workspace_bytes(Q, n, kq)


@_on_device
def lstsq_rows(Rt, ids, C, ridge=0.0, max_bytes=LSTSQ_WS_LIMIT_BYTES, out=None, timings=None):
	"""Per-query least squares (anncur_lstsq_rows): row q of W = argmin_w ||w R_S - C[q]||^2 + ridge ||w||^2 with R_S the columns
	Rt[ids[q, j], :]^T, j over the non-holes -- at ridge = 0 and full rank, C[q] . pinv(R_S).  Rt [m x kq] fp32 (rows may be padded),
	ids int32 [Q x n] (-1 = hole, distinct within a row), C fp32 [Q x n].  -> (W fp32 [Q x kq], status int32 [Q]); status[q] = 1 and a NaN
	row where a Cholesky pivot fell to 2^-40 max diag(G) or below (the pivot rule of include/anncur_hip.h).
	The workspace is one grow-only buffer per device; above max_bytes the queries run in chunks (at least one query per chunk).
	out: (W, status) to fill.  timings: a list that receives one (gram_ms, factor_ms, matvec_ms) tuple per chunk (synchronises)."""
	_dev(Rt, ids, C)
	if Rt.dtype != torch.float32 or C.dtype != torch.float32:
		raise TypeError("lstsq_rows takes float32 Rt and C")
	if ids.dim() != 2 or C.dim() != 2 or tuple(ids.shape) != tuple(C.shape) or Rt.dim() != 2:
		raise ValueError("lstsq_rows: Rt [m x kq], ids and C [Q x n] of one shape")
	if ids.dtype != torch.int32:
		raise ValueError(f"lstsq_rows: ids must be int32 (got {ids.dtype})")
	Rt, ids, C = _rowmajor(Rt), _rowmajor(ids), _rowmajor(C)
	(m, kq), (Q, n) = Rt.shape, ids.shape
	ridge = float(ridge)
	_lstsq_check(Q, n, kq, ridge)
	if out is None:
		W = torch.empty((Q, kq), dtype=torch.float32, device=Rt.device)
		status = torch.empty((Q,), dtype=torch.int32, device=Rt.device)
	else:
		W, status = out
		if tuple(W.shape) != (Q, kq) or W.dtype != torch.float32 or (kq > 1 and W.stride(1) != 1) or tuple(status.shape) != (Q,) or status.dtype != torch.int32 \
				or not status.is_contiguous() or W.device != Rt.device or status.device != Rt.device:
			raise ValueError("lstsq_rows: out = (W fp32 [Q x kq] with unit column stride, status int32 [Q] contiguous) on Rt's device")
	if Q == 0:
		return W, status
	lib = _lib.load()
	per_query = lib.anncur_lstsq_rows_workspace_bytes(1, n, kq)
	g = min(n, kq)
	nt = -(-g // 64)
	qc = max(1, min(Q, int(max_bytes) // per_query, (0x7fffffff - 1) // max(nt * (nt + 1) // 2, -(-kq // 64) + 1)))
	ws = _Workspace.get(lib.anncur_lstsq_rows_workspace_bytes(qc, n, kq), Rt.device)
	for q0 in range(0, Q, qc):
		q1 = min(Q, q0 + qc)
		args = (_p(Rt), _ld(Rt), m, kq, _p(ids[q0:q1]), _ld(ids), _p(C[q0:q1]), _ld(C), q1 - q0, n, ridge, _p(W[q0:q1]), _ld(W) if Q > 1 else kq,
				_p(status[q0:q1]), _p(ws), ws.numel(), _stream())
		if timings is None:
			check(lib.anncur_lstsq_rows(*args), "lstsq_rows")
		else:
			ms = (ctypes.c_float * 3)()
			check(lib.anncur_lstsq_rows_timed(*args, ms), "lstsq_rows_timed")
			timings.append(tuple(ms))
	return W, status


LSTSQ_STATE_LIMIT_BYTES = 32 << 30   # default cap of one LstsqState: a policy, not a measurement (10 000 queries at cap = 456 take 17 GB)


def lstsq_state_bytes(Q, cap):
	"""Bytes of the persistent state of anncur_lstsq_extend for Q queries of up to cap scored items (0 outside its limits)."""
	return _lib.load().anncur_lstsq_state_bytes(Q, cap)


class LstsqState(object):
	"""lstsq_rows for id lists that only grow at the end (anncur_lstsq_extend, item side): the Gram matrix, its Cholesky factor and the
	forward-substituted right-hand side of every query stay in one device buffer that this object owns (not the shared grow-only
	workspace, which other calls overwrite), and extend() pays for the appended positions only.  Rt [m x kq] fp32, Q queries, at most
	cap <= ANNCUR_LSTSQ_MAX_G positions per query; ridge is fixed for the state's life.  After every extend(ids, C) the result equals
	lstsq_rows(Rt, ids, C, ridge) bit for bit, status included; a query that failed once (status 1, NaN row) stays failed.
	seed_shared(shared_ids), on a fresh state, factors a prefix that all queries share once instead of once per query (same results).
	.n = the positions absorbed so far, .cap.  Every limit is a ValueError that names it, raised before any launch."""

	def __init__(self, Rt, Q, cap, ridge=0.0, max_bytes=LSTSQ_STATE_LIMIT_BYTES):
		if not torch.is_tensor(Rt) or Rt.dim() != 2 or Rt.dtype != torch.float32:
			raise ValueError("LstsqState: Rt must be a float32 tensor [m x kq]")
		Q, cap, ridge = int(Q), int(cap), float(ridge)
		kq = Rt.shape[1]
		if cap < 1 or cap > _lib.LSTSQ_MAX_G:
			raise ValueError(f"LstsqState: cap = {cap} scored items per query, outside 1..ANNCUR_LSTSQ_MAX_G = {_lib.LSTSQ_MAX_G}")
		if kq < 1 or kq > _lib.LSTSQ_MAX_KQ:
			raise ValueError(f"LstsqState: kq = {kq} anchor queries, outside 1..ANNCUR_LSTSQ_MAX_KQ = {_lib.LSTSQ_MAX_KQ}")
		if Q < 0:
			raise ValueError(f"LstsqState: Q = {Q} queries")
		if not ridge >= 0.0:
			raise ValueError(f"LstsqState: ridge = {ridge}, need ridge >= 0")
		self.nbytes = _lib.load().anncur_lstsq_state_bytes(Q, cap)
		if self.nbytes > int(max_bytes):
			raise ValueError(f"LstsqState: {Q} queries at cap = {cap} need {self.nbytes} bytes of state, above max_bytes = {int(max_bytes)}: "
							 f"search the queries in batches")
		self.Rt, self.Q, self.cap, self.kq, self.ridge, self.n = Rt, Q, cap, kq, ridge, 0
		self._buf = None      # allocated by the first extend

	def _state(self):
		if self._buf is None:
			self._buf = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=self.Rt.device)
		off = (-self._buf.data_ptr()) % 256
		return self._buf[off:off + self.nbytes]

	def seed_shared(self, shared_ids):
		"""Start the state from a prefix that EVERY query's rows begin with (anncur_lstsq_seed_shared; the adaptive search's anchor items):
		the prefix is factored once, for one query, and copied to the others, so the first extend() pays for the positions after it only.
		shared_ids: a host list, numpy array or int32 tensor of n_sh ids, in the order in which the rows hold them (the caller's contract, as
		for extend).  Afterwards .n = n_sh; every extend() returns what it returns on an unseeded state, bit for bit.  Duplicates are not an
		error: they are rank deficiency and fail every query through the status of the first extend.  ValueError, before any launch: the
		state has absorbed something already, n_sh outside 1..min(cap, kq), an id outside [0, m) (ids given on the GPU are taken as they
		are: checking them would cost a synchronisation).  No host synchronisation."""
		if self.n != 0:
			raise ValueError(f"LstsqState.seed_shared: {self.n} positions are absorbed already: a state is seeded before its first extend (.n == 0)")
		on_gpu = torch.is_tensor(shared_ids) and shared_ids.is_cuda
		if on_gpu:
			if shared_ids.dim() != 1 or shared_ids.dtype != torch.int32:
				raise ValueError(f"LstsqState.seed_shared: shared_ids on the GPU must be a flat int32 tensor (got {shared_ids.dtype}, {shared_ids.dim()}-D)")
			n_sh = shared_ids.shape[0]
		else:
			a = np.asarray(shared_ids.detach().numpy() if torch.is_tensor(shared_ids) else shared_ids)
			if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
				raise ValueError("LstsqState.seed_shared: shared_ids must be a flat list of integer item ids")
			a = a.astype(np.int64)
			n_sh = int(a.size)
		if n_sh < 1 or n_sh > min(self.cap, self.kq):
			raise ValueError(f"LstsqState.seed_shared: n_sh = {n_sh} shared ids, outside 1..min(cap, kq) = min({self.cap}, {self.kq}) = {min(self.cap, self.kq)}")
		m = self.Rt.shape[0]
		if not on_gpu and (int(a.min()) < 0 or int(a.max()) >= m):
			bad = int(a.min()) if int(a.min()) < 0 else int(a.max())
			raise ValueError(f"LstsqState.seed_shared: id {bad} outside [0, m) = [0, {m}): a shared id names an item (holes belong to the appended positions)")
		_dev(self.Rt)
		if on_gpu and shared_ids.device != self.Rt.device:
			raise _lib.AnncurHipError(f"LstsqState.seed_shared: operands live on different devices (Rt on {self.Rt.device}, shared_ids on {shared_ids.device})")
		ids = shared_ids.contiguous() if on_gpu else torch.from_numpy(a.astype(np.int32)).to(self.Rt.device)
		self._seed(ids, n_sh)

	@_on_device
	def _seed(self, ids, n_sh):
		Rt = _rowmajor(self.Rt)
		if self.Q:
			if (self.Q - 1) * -(-n_sh // 16) >= 0x7fffffff:
				raise ValueError(f"LstsqState.seed_shared: Q = {self.Q} queries are too many for one launch at this size: search the queries in batches")
			st = self._state()
			check(_lib.load().anncur_lstsq_seed_shared(_p(Rt), _ld(Rt), Rt.shape[0], self.kq, _p(ids), n_sh, self.Q, self.cap, self.ridge, _p(st), st.numel(),
													   _stream()), "lstsq_seed_shared")
		self.n = n_sh

	def extend(self, ids, C, out=None, timings=None):
		"""ids int32 / C fp32 [Q x n], n > .n: the FULL rows in insertion order, whose first .n positions are what the last call saw (the
		caller's contract).  -> (W fp32 [Q x kq], status int32 [Q]) as lstsq_rows returns them for these rows.  out: (W, status) to fill.
		timings: a list that receives one (gram_ms, factor_ms, matvec_ms) tuple (synchronises)."""
		if not (torch.is_tensor(ids) and torch.is_tensor(C)) or ids.dim() != 2 or C.dim() != 2 or tuple(ids.shape) != tuple(C.shape) \
				or ids.shape[0] != self.Q or ids.dtype != torch.int32 or C.dtype != torch.float32:
			raise ValueError(f"LstsqState.extend: ids int32 and C float32, both [Q x n] of one shape with Q = {self.Q}")
		n = ids.shape[1]
		if n <= self.n:
			raise ValueError(f"LstsqState.extend: rows of {n} positions, but {self.n} are absorbed already: a call appends at least one (the lists never shrink)")
		if n > self.cap:
			raise ValueError(f"LstsqState.extend: rows of {n} positions, above this state's cap = {self.cap}")
		if n > self.kq:
			raise ValueError(f"LstsqState.extend: rows of {n} positions, above kq = {self.kq} anchor queries: the query side has no incremental form "
							 f"(lstsq_rows solves it)")
		if ids.device != self.Rt.device or C.device != self.Rt.device:
			raise _lib.AnncurHipError(f"LstsqState.extend: operands live on different devices (Rt on {self.Rt.device}, ids on {ids.device}, C on {C.device})")
		return self._extend(ids, C, n, out, timings)

	@_on_device
	def _extend(self, ids, C, n, out, timings):
		_dev(self.Rt, ids, C)
		Rt, ids, C = _rowmajor(self.Rt), _rowmajor(ids), _rowmajor(C)
		Q, kq = self.Q, self.kq
		if out is None:
			W = torch.empty((Q, kq), dtype=torch.float32, device=Rt.device)
			status = torch.empty((Q,), dtype=torch.int32, device=Rt.device)
		else:
			W, status = out
			if tuple(W.shape) != (Q, kq) or W.dtype != torch.float32 or (kq > 1 and W.stride(1) != 1) or tuple(status.shape) != (Q,) or status.dtype != torch.int32 \
					or not status.is_contiguous() or W.device != Rt.device or status.device != Rt.device:
				raise ValueError("LstsqState.extend: out = (W fp32 [Q x kq] with unit column stride, status int32 [Q] contiguous) on Rt's device")
		if Q:
			nt = -(-n // 64)
			if Q * max(nt * (nt + 1) // 2, -(-kq // 64)) >= 0x7fffffff:
				raise ValueError(f"LstsqState.extend: Q = {Q} queries are too many for one launch at this size: search the queries in batches")
			lib, st = _lib.load(), self._state()
			args = (_p(Rt), _ld(Rt), Rt.shape[0], kq, _p(ids), _ld(ids), _p(C), _ld(C), Q, self.n, n, self.cap, self.ridge, _p(W), _ld(W), _p(status),
					_p(st), st.numel(), _stream())
			if timings is None:
				check(lib.anncur_lstsq_extend(*args), "lstsq_extend")
			else:
				ms = (ctypes.c_float * 3)()
				check(lib.anncur_lstsq_extend_timed(*args, ms), "lstsq_extend_timed")
				timings.append(tuple(ms))
		self.n = n
		return W, status


@_on_device
def sort_id_rows(ids, scores, out=None):
	"""Rows of (id int32, score fp32) pairs [Q x w] sorted ascending by id, holes (id < 0) last, scores carried along, equal ids in their
	input order (anncur_sort_id_rows).  -> (ids, scores, counts int32 [Q] = non-holes per row).  out = (ids, scores) to fill; may be the
	inputs."""
	_dev(ids, scores)
	if ids.dim() != 2 or tuple(ids.shape) != tuple(scores.shape):
		raise ValueError("sort_id_rows: ids and scores must be 2-D tensors [Q x w] of one shape")
	if ids.dtype != torch.int32 or scores.dtype != torch.float32:
		raise ValueError(f"sort_id_rows: ids int32 and scores float32 (got {ids.dtype}, {scores.dtype})")
	Q, w = ids.shape
	if w < 1 or w > _lib.MAX_TOPK:
		raise ValueError(f"sort_id_rows: rows of {w} pairs, outside 1..ANNCUR_MAX_TOPK = {_lib.MAX_TOPK}")
	ids, scores = _rowmajor(ids), _rowmajor(scores)
	if _ld(ids) != _ld(scores):
		ids, scores = ids.contiguous(), scores.contiguous()
	if out is None:
		out = (torch.empty((Q, w), dtype=torch.int32, device=ids.device), torch.empty((Q, w), dtype=torch.float32, device=ids.device))
	o_ids, o_sc = out
	if tuple(o_ids.shape) != (Q, w) or tuple(o_sc.shape) != (Q, w) or o_ids.dtype != torch.int32 or o_sc.dtype != torch.float32 or _ld(o_ids) != _ld(o_sc) \
			or (w > 1 and (o_ids.stride(1) != 1 or o_sc.stride(1) != 1)):
		raise ValueError("sort_id_rows: out = (ids int32, scores float32), both [Q x w] with unit column stride and one row pitch")
	counts = torch.empty((Q,), dtype=torch.int32, device=ids.device)
	check(_lib.load().anncur_sort_id_rows(_p(ids), _p(scores), _ld(ids), Q, w, _p(o_ids), _p(o_sc), _ld(o_ids), _p(counts), _stream()), "sort_id_rows")
	return o_ids, o_sc, counts


def exclusion_from_sorted_rows(ids_sorted, counts=None):
	"""Exclusion(off, ids, e_max) of exclusion() from rows that sort_id_rows sorted and that are FULL (no hole): row q is query q's list,
	off = arange(Q + 1) w, e_max = w -- built on the device, where exclusion() would copy the rows to the host and numpy.unique each.
	Rows with a hole are refused (ValueError): the one host look is a single flag, from `counts` (sort_id_rows' third result) or, without
	it, from the last id of each row (holes sort last).  The ids must be distinct within a row; that is the caller's contract."""
	_dev(ids_sorted)
	if ids_sorted.dim() != 2 or ids_sorted.dtype != torch.int32:
		raise ValueError("exclusion_from_sorted_rows: ids_sorted must be an int32 tensor [Q x w]")
	Q, w = ids_sorted.shape
	if Q and w:
		holes = (counts != w).any() if counts is not None else (ids_sorted[:, -1] < 0).any()
		if bool(holes.item()):
			raise ValueError(f"exclusion_from_sorted_rows: a row holds fewer than w = {w} ids (a hole); exclusion() takes padded rows")
	off = torch.arange(Q + 1, dtype=torch.int64, device=ids_sorted.device) * w
	return Exclusion(off, ids_sorted.contiguous().view(-1), int(w) if Q else 0)


# ------------------------------------------------------------------ anchor item selection
def _select_pivoted_check(kq, m, k):
	"""The limits of anncur_select_pivoted, as ValueErrors that name them (nothing needs a GPU here)."""
	if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
		raise ValueError(f"select_pivoted: k must be an integer (got {k!r})")
	if kq < 1 or kq > _lib.LSTSQ_MAX_KQ:
		raise ValueError(f"select_pivoted: kq = {kq} anchor queries, outside 1..ANNCUR_LSTSQ_MAX_KQ = {_lib.LSTSQ_MAX_KQ}")
	if m >= 1 << 31:
		raise ValueError(f"select_pivoted: m = {m} items, need m < 2^31")
	lim = min(kq, m, _lib.MAX_TOPK)
	if k < 1 or k > lim:
		raise ValueError(f"select_pivoted: k = {k} outside 1..min(kq, items, ANNCUR_MAX_TOPK) = min({kq}, {m}, {_lib.MAX_TOPK}) = {lim}")


def select_pivoted_slice_items(dtype):
	"""Items per slice of anncur_select_pivoted's step kernel for a torch dtype (what one workgroup covers per turn): for tests of its edges."""
	return int(_lib.load().anncur_select_pivoted_slice_items(_DT[dtype]))


@_on_device
def select_pivoted(R, k):
	"""Column-pivoted QR selection of k items from the anchor rows R [kq x m] (fp32 or bf16, rows may be padded; anncur_select_pivoted,
	whose contract is in include/anncur_hip.h): -> (ids int32 [k] in SELECTION order, gains float64 [k] = the squared residual norm each had
	when taken, n_sel int).  Positions >= n_sel hold (-1, 0.0): the selection stopped at the numerical rank (lstsq_rows' pivot rule).  The
	first k' entries are the result for k' < k.  One grow-only workspace per device; the one host look is n_sel."""
	if not torch.is_tensor(R) or R.dim() != 2:
		raise ValueError("select_pivoted: R must be a 2-D tensor [kq x m]")
	kq, m = R.shape
	_select_pivoted_check(kq, m, k)
	_dev(R)
	dt = _dt(R)
	R = _rowmajor(R)
	lib = _lib.load()
	ids = torch.empty((k,), dtype=torch.int32, device=R.device)
	gains = torch.empty((k,), dtype=torch.float64, device=R.device)
	n_sel = torch.empty((1,), dtype=torch.int32, device=R.device)
	ws = _Workspace.get(lib.anncur_select_pivoted_workspace_bytes(m, kq, k), R.device)
	check(lib.anncur_select_pivoted(_p(R), dt, _ld(R), kq, m, int(k), _p(ids), _p(gains), _p(n_sel), _p(ws), ws.numel(), _stream()), "select_pivoted")
	return ids, gains, int(n_sel.item())


# ------------------------------------------------------------------ Jacobi SVD and the truncated pseudo-inverse
SVD = namedtuple("SVD", ["U", "S", "V", "sweeps", "converged"])


def _svd_check(rows, cols):
	"""The limits of anncur_svd_*, as ValueErrors that name them (nothing needs a GPU here)."""
	g, L = min(rows, cols), max(rows, cols)
	if g < 1 or g > _lib.SVD_MAX_G:
		raise ValueError(f"svd_jacobi: min(rows, cols) = {g} outside 1..ANNCUR_SVD_MAX_G = {_lib.SVD_MAX_G} (block {rows} x {cols})")
	if L > _lib.SVD_MAX_L:
		raise ValueError(f"svd_jacobi: max(rows, cols) = {L} above ANNCUR_SVD_MAX_L = {_lib.SVD_MAX_L} (block {rows} x {cols})")


def _rcond_check(rcond, what):
	"""rcond of a truncated pseudo-inverse: a number in [0, 1) (numpy.linalg.pinv's cutoff relative to the largest singular value)."""
	try:
		r = float(rcond)
	except (TypeError, ValueError):
		raise ValueError(f"{what}: rcond must be a number in [0, 1) (got {rcond!r})") from None
	if not (0.0 <= r < 1.0):
		raise ValueError(f"{what}: rcond = {rcond!r} outside [0, 1)")
	return r


@_on_device
def svd_jacobi_unsorted(W, max_sweeps=30, workspace=None, out=None):
	"""The three C calls of the Jacobi SVD around the convergence loop: anncur_svd_init, then anncur_svd_sweep until a sweep rotates nothing or
	max_sweeps have run (one 4-byte read of the counter per sweep, the loop's only synchronisation), then anncur_svd_finish.
	-> (sigma fp64 [g] in the workspace's order, U fp64 [rows x g], V fp64 [cols x g], sweeps, converged).
	workspace: a 256-byte aligned uint8 tensor of at least anncur_svd_workspace_bytes (default: the grow-only scratch of the device).
	out: (sigma, U, V, rotations int32 [1], flag int32 [1]) to write into (U, V with unit column stride and any row pitch >= g); default: fresh tensors."""
	if not torch.is_tensor(W) or W.dim() != 2:
		raise ValueError("svd_jacobi: W must be a 2-D tensor")
	rows, cols = W.shape
	_svd_check(rows, cols)
	if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or max_sweeps < 1:
		raise ValueError(f"svd_jacobi: max_sweeps must be an integer >= 1 (got {max_sweeps!r})")
	_dev(W)
	dt = _dt(W)
	W = _rowmajor(W)
	g = min(rows, cols)
	lib = _lib.load()
	need = lib.anncur_svd_workspace_bytes(rows, cols)
	ws = _Workspace.get(need, W.device) if workspace is None else workspace
	if out is None:
		out = (torch.empty((g,), dtype=torch.float64, device=W.device), torch.empty((rows, g), dtype=torch.float64, device=W.device),
			   torch.empty((cols, g), dtype=torch.float64, device=W.device), torch.empty((1,), dtype=torch.int32, device=W.device),
			   torch.empty((1,), dtype=torch.int32, device=W.device))
	sigma, U, V, rot, flag = out
	if tuple(U.shape) != (rows, g) or tuple(V.shape) != (cols, g) or sigma.numel() != g or any(t.dtype != torch.float64 for t in (sigma, U, V)) or \
			(g > 1 and (U.stride(1) != 1 or V.stride(1) != 1)) or not sigma.is_contiguous():
		raise ValueError("svd_jacobi: out = (sigma fp64 [g], U fp64 [rows x g], V fp64 [cols x g], rotations int32 [1], flag int32 [1]), unit column strides")
	check(lib.anncur_svd_init(_p(W), dt, _ld(W), rows, cols, _p(ws), ws.numel(), _stream()), "svd_init")
	sweeps, converged = 0, False
	while sweeps < max_sweeps and not converged:
		check(lib.anncur_svd_sweep(rows, cols, _p(ws), ws.numel(), _p(rot), _stream()), "svd_sweep")
		sweeps += 1
		converged = int(rot.item()) == 0
	check(lib.anncur_svd_finish(rows, cols, _p(ws), ws.numel(), _p(sigma), _p(U), max(_ld(U), g), _p(V), max(_ld(V), g), _p(flag), _stream()), "svd_finish")
	if int(flag.item()) != 0:
		converged = False   # a singular value that is not finite: W held a NaN / inf, or a norm left the fp64 range
	return sigma, U, V, sweeps, converged


def svd_jacobi(W, max_sweeps=30):
	"""Singular value decomposition of ONE block W [rows x cols] (fp32 or bf16 on the GPU, any row pitch) by one-sided Jacobi rotations in fp64
	(anncur_svd_*; include/anncur_hip.h has the contract) -> SVD(U fp64 [rows x g], S fp64 [g] DESCENDING, V fp64 [cols x g], sweeps, converged),
	g = min(rows, cols), W = U diag(S) V^T.  converged: a whole sweep rotated nothing; otherwise the call stops after max_sweeps sweeps and says
	so (no exception); a singular value that is not finite also gives converged = False.  Limits: 1 <= g <= ANNCUR_SVD_MAX_G = 2048,
	max(rows, cols) <= ANNCUR_SVD_MAX_L = 8192 (ValueError, before any launch).  The same input gives the same bits on every run.
	The kernels leave the singular values in the order of W's vectors; the sort (stable, descending) and the matching column permutation of U
	and V are torch indexing, not arithmetic."""
	sigma, U, V, sweeps, converged = svd_jacobi_unsorted(W, max_sweeps)
	S, order = torch.sort(sigma, descending=True, stable=True)
	return SVD(U.index_select(1, order), S, V.index_select(1, order), sweeps, converged)


def pinv_from_svd(svd, rcond=1e-15):
	"""Truncated pseudo-inverse from a decomposition: X = sum over sigma_i > rcond sigma_max of v_i u_i^T / sigma_i (numpy.linalg.pinv's rule),
	summed in fp64 (anncur_svd_scale_cols, then anncur_gemm_f64) and rounded to fp32 once -> (X fp32 [cols x rows], rank = the number of
	singular values kept).  One decomposition serves any number of cutoffs: a call costs one small GEMM.  rcond in [0, 1), else ValueError."""
	rcond = _rcond_check(rcond, "pinv_from_svd")
	return _pinv_from_svd(svd.U, svd.S, svd.V, rcond)


@_on_device
def _pinv_from_svd(U, S, V, rcond):
	_dev(U, S, V)
	cols, g = V.shape
	rows = U.shape[0]
	if any(t.dtype != torch.float64 for t in (U, S, V)) or U.shape[1] != g or S.numel() != g:
		raise ValueError("pinv_from_svd: need U fp64 [rows x g], S fp64 [g], V fp64 [cols x g]")
	V, S = _rowmajor(V), S.contiguous()
	Vs = torch.empty((cols, g), dtype=torch.float64, device=V.device)
	rank = torch.empty((1,), dtype=torch.int32, device=V.device)
	check(_lib.load().anncur_svd_scale_cols(_p(V), max(_ld(V), g), cols, g, _p(S), rcond, _p(Vs), g, _p(rank), _stream()), "svd_scale_cols")
	X64 = gemm_f64(Vs, U.t())                                # [cols x rows]
	X = torch.empty((cols, rows), dtype=torch.float32, device=V.device)
	convert_f64(X64, X)
	return X, int(rank.item())


@_on_device
def gather_pairs(A, idx):
	"""out[q, j] = A[q, idx[q, j]] as float32 [Q x n]; an id outside [0, I) (a hole) gives NaN (reference: ..._splits.py:91-96 reads
	these cells of the exact matrix)."""
	_dev(A, idx)
	A = _rowmajor(A)
	if idx.dim() != 2 or idx.shape[0] != A.shape[0]:
		raise ValueError(f"gather_pairs: idx must be a 2-D tensor with one row per row of A ({A.shape[0]})")
	if idx.dtype != torch.int32:
		idx = idx.to(torch.int32)
	idx = _rowmajor(idx)
	Q, n = idx.shape
	out = torch.empty((Q, n), dtype=torch.float32, device=A.device)
	check(_lib.load().anncur_gather_pairs(_p(A), _dt(A), Q, A.shape[1], _ld(A), _p(idx), _ld(idx), n, _p(out), max(n, 1), _stream()), "gather_pairs")
	return out


@_on_device
def overlap_counts(a, b, pairs, mapped_host_out=None):
	"""common[p, q] = |set(a[q, :ka_p]) & set(b[q, :kb_p])| for pairs = [(ka, kb), ...] -> int32 [n_pairs, Q].
	Ids below zero (the -1 pads of a short top-k row) belong to no set; either list may repeat an id, which counts once, at its first position
	in each list.  Lists hold 1..4096 ids; any number of pairs (64 per launch, each launch writing its own rows of the result); pairs = [] or
	Q = 0 give the empty result without a launch.
	mapped_host_out: a contiguous PINNED host tensor int32 [n_pairs, Q] (mapped into the device address space by the HIP runtime): the kernel writes
	the counts there itself -- no device buffer, no copy launch (graph-capturable; the caller synchronises before reading it).  Every element is
	written; it is also what the call returns."""
	Q = a.shape[0]
	if mapped_host_out is not None:
		out = mapped_host_out
		if out.is_cuda or not out.is_pinned() or not out.is_contiguous() or out.dtype != torch.int32 or tuple(out.shape) != (len(pairs), Q):
			raise ValueError("overlap_counts: mapped_host_out must be a contiguous pinned int32 host tensor [n_pairs, Q]")
	_dev(a, b)
	a = a.to(torch.int32).contiguous()
	b = b.to(torch.int32).contiguous()
	if mapped_host_out is None:
		out = torch.empty((len(pairs), Q), dtype=torch.int32, device=a.device)
	lib = _lib.load()
	for s in range(0, len(pairs), 64):
		chunk = pairs[s:s + 64]
		ka = (ctypes.c_int32 * len(chunk))(*[int(p[0]) for p in chunk])
		kb = (ctypes.c_int32 * len(chunk))(*[int(p[1]) for p in chunk])
		check(lib.anncur_overlap_counts(_p(a), a.shape[1], _p(b), b.shape[1], Q, ka, kb, len(chunk), _p(out[s:s + len(chunk)]), _stream()),
			  "overlap_counts")
	return out


# ------------------------------------------------------------------ f3: inverted file
@_on_device
def ivf_build_lists(assign, nlist):
	"""assign int32 [n] -> (counts int32 [nlist], offsets int32 [nlist + 1], ids int32 [n]: the points of each list, ascending)."""
	_dev(assign)
	assign = assign.to(torch.int32).contiguous()
	n = assign.numel()
	counts = torch.empty(nlist, dtype=torch.int32, device=assign.device)
	offsets = torch.empty(nlist + 1, dtype=torch.int32, device=assign.device)
	ids = torch.empty(n, dtype=torch.int32, device=assign.device)
	check(_lib.load().anncur_ivf_build_lists(_p(assign), n, nlist, _p(counts), _p(offsets), _p(ids), _stream()), "ivf_build_lists")
	return counts, offsets, ids


@_on_device
def descending_norm_order(M, n_buckets=256):
	"""Row ids of the fp32 matrix M in coarse descending-norm order (int32 device tensor): norm buckets + the stable counting sort
	of the inverted-file builder.  The index builder's ordering hint; no torch arithmetic involved."""
	_dev(M)
	M = _rowmajor(M)
	if M.dtype != torch.float32:
		raise TypeError("descending_norm_order takes fp32")
	n = M.shape[0]
	norms = torch.empty(n, dtype=torch.float32, device=M.device)
	mm = torch.empty(2, dtype=torch.int32, device=M.device)
	bucket = torch.empty(n, dtype=torch.int32, device=M.device)
	check(_lib.load().anncur_norm_buckets(_p(M), n, M.shape[1], _ld(M), n_buckets, _p(norms), _p(mm), _p(bucket), _stream()), "norm_buckets")
	return ivf_build_lists(bucket, n_buckets)[2]


@_on_device
def ivf_list_means(Xs, offsets, centroids):
	"""centroids[l] <- mean of the rows of list l of Xs (list-ordered fp32 vectors); empty lists keep theirs.  In place."""
	_dev(Xs, offsets, centroids)
	Xs = _rowmajor(Xs)
	if Xs.dtype != torch.float32 or centroids.dtype != torch.float32 or centroids.stride(1) != 1:
		raise TypeError("ivf_list_means takes fp32 row-major tensors")
	check(_lib.load().anncur_ivf_list_means(_p(Xs), _ld(Xs), centroids.shape[1], _p(offsets), centroids.shape[0], _p(centroids), _ld(centroids), _stream()),
		  "ivf_list_means")
	return centroids


@_on_device
def renorm_rows(M):
	"""Rows of the fp32 matrix M rescaled to unit L2 norm, in place (a zero row stays): FAISS' fvec_renorm_L2 (spherical k-means)."""
	_dev(M)
	if M.dtype != torch.float32 or M.dim() != 2 or (M.shape[1] > 1 and M.stride(1) != 1):
		raise TypeError("renorm_rows takes a row-major fp32 matrix")
	check(_lib.load().anncur_renorm_rows(_p(M), M.shape[0], M.shape[1], _ld(M), _stream()), "renorm_rows")
	return M


@_on_device
def ivf_scan(Xs, offsets, ids, Q, probe, k):
	"""Exact inner products inside the probed lists + top-k.  Xs [n x dp], Q [nq x dp] fp32 zero-padded to dp (multiple of 16)."""
	_dev(Xs, offsets, ids, Q, probe)
	nq, dp = Q.shape
	probe = probe.to(torch.int32).contiguous()
	val = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
	idx = torch.empty((nq, k), dtype=torch.int32, device=Q.device)
	check(_lib.load().anncur_ivf_scan(_p(Xs), _ld(Xs), dp, _p(offsets), _p(ids), _p(Q), _ld(Q), nq, _p(probe), probe.shape[1], k, _p(val), _p(idx), _stream()),
		  "ivf_scan")
	return TopK(val, idx)


def _ivf_max_tiles(n_pairs, sizes_host, T):
	"""An upper bound on the number of T-pair x T-vector tiles of a batched search that needs no look at the pairs-per-list counts (they stay
	on the device: no synchronisation inside a search): sum_l ceil(pairs_l / T) vt_l <= (pairs // T) max_l vt_l + sum_l vt_l, vt_l =
	ceil(size_l / T).  Workgroups past the last tile exit."""
	vt = -(-sizes_host // T)
	return (n_pairs // T) * int(max(int(vt.max()), 1)) + int(vt.sum())


def _ivf_chunked(nq_all, step, k, k_eff, device, run):
	"""The query-chunk loop of the batched searches: run(q0, q1, out_val, out_idx) fills the [q1 - q0 x k_eff] results of queries q0 .. q1 - 1
	-- rows of the [nq_all x k] outputs themselves when k_eff == k, temporaries otherwise: no more than k_eff vectors can be found, and the
	rows' tails are (-inf, -1)."""
	val = torch.empty((nq_all, k), dtype=torch.float32, device=device)
	idx = torch.empty((nq_all, k), dtype=torch.int32, device=device)
	for q0 in range(0, nq_all, step):
		q1 = min(nq_all, q0 + step)
		if k_eff == k:
			run(q0, q1, val[q0:q1], idx[q0:q1])
			continue
		ov = torch.empty((q1 - q0, k_eff), dtype=torch.float32, device=device)
		oi = torch.empty((q1 - q0, k_eff), dtype=torch.int32, device=device)
		run(q0, q1, ov, oi)
		val[q0:q1, :k_eff] = ov; idx[q0:q1, :k_eff] = oi
		val[q0:q1, k_eff:] = float("-inf"); idx[q0:q1, k_eff:] = -1
	return TopK(val, idx)


@_on_device
def ivf_scan_grouped(Xs, offsets, ids, sizes_host, Q, probe, k, max_bytes=8 << 30, lists_bf16=None, profile=None):
	"""The same search as ivf_scan for MANY queries: pairs (query, probe slot) sorted by list, every list one small MFMA GEMM against its
	pairs' queries (anncur_ivf_group_scores_dev), then the exact scan over each query's nprobe lists side by side and the column -> id map.
	sizes_host: the lists' lengths on the host (numpy int64, known since add()); they bound the tile count of the launch, the worklist itself is
	built on the device (no synchronisation inside the call: the search is stream-ordered like every other op).
	lists_bf16: a bf16 copy of Xs (same layout) -> the per-list GEMMs run on the bf16 matrix cores (queries rounded to bf16 here).
	profile: a dict -> receives HIP events around the per-list GEMM launch and around the scan + id map ("events": [(e0, e1, e2), ...] per
	query chunk; measurement only: bench.py's kernel-only IVF figure)."""
	_dev(Xs, offsets, ids, Q, probe)
	lib = _lib.load()
	nq_all, dp = Q.shape
	probe = probe.to(torch.int32).contiguous()
	nprobe, nlist = probe.shape[1], sizes_host.shape[0]
	lmax = -(-max(int(sizes_host.max()), 1) // 8) * 8
	lists = Xs if lists_bf16 is None else lists_bf16

	def run(q0, q1, ov, oi):
		nq, k_eff = ov.shape
		pr = probe[q0:q1].contiguous()
		cnt, poff, pair_ids = ivf_build_lists(pr.reshape(-1).clamp(min=0), nlist)     # (probe slots are valid list ids here: nprobe <= nlist)
		max_tiles = _ivf_max_tiles(nq * nprobe, sizes_host, 64)
		tile_start = torch.empty(nlist + 1, dtype=torch.int32, device=Q.device)
		S = _ScoreScratch.get(nq * nprobe * lmax, Q.device).view(nq, nprobe * lmax)   # grow-only scratch: a fresh 100s-of-MB allocation per call cost more than the search
		S.fill_(float("-inf"))
		if profile is not None:
			evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
			profile.setdefault("events", []).append(evs)
			profile.setdefault("max_tiles", []).append(int(max_tiles))
			profile.setdefault("tile_starts", []).append(tile_start)
			evs[0].record()
		Qc = Q[q0:q1] if lists_bf16 is None else convert(Q[q0:q1], torch.bfloat16)
		check(lib.anncur_ivf_group_scores_dev(_p(lists), _dt(lists), _ld(lists), dp, _p(offsets), nlist, _p(Qc), _ld(Qc), nprobe, _p(pair_ids), _p(poff),
											  _p(tile_start), max_tiles, lmax, _p(S), _stream()), "ivf_group_scores_dev")
		if profile is not None: evs[1].record()
		v, c = rowwise_topk(S, k_eff)
		check(lib.anncur_ivf_map_ids(_p(c), _p(v), nq, k_eff, lmax, _p(pr), nprobe, _p(offsets), _p(ids), _p(oi), _stream()), "ivf_map_ids")
		if profile is not None: evs[2].record()
		ov.copy_(v)

	step = max(64, min(nq_all, max_bytes // (nprobe * lmax * 4)))
	return _ivf_chunked(nq_all, step, k, min(k, nprobe * lmax), Q.device, run)


IVF_GROUPED_MAX_K, IVF_GROUPED_MAX_NLIST = 128, 8192


def ivf_search_grouped_ok(k, nlist):
	"""True where ivf_search_grouped serves the search (the wave-per-row scan's k, list histograms in LDS); ivf_scan_grouped otherwise."""
	return k <= IVF_GROUPED_MAX_K and nlist <= IVF_GROUPED_MAX_NLIST


@_on_device
def ivf_search_grouped(lists, offsets, ids, sizes_host, Q, probe, k, max_bytes=8 << 30, _skip_gemm=False):
	"""The batched IVF search of ivf_scan_grouped as ONE library call per query chunk (round 5): pairs grouped by list on the device, one tile
	GEMM launch on the matrix cores (bf16 `lists` / Q with rows a multiple of 128 elements: 128 x 128 tiles), scores in PACKED rows (query q's
	probed lists back to back, nothing pre-filled), ragged scan, column -> id map.  lists / Q: fp32 or bf16 (the same for both), rows
	zero-padded to a multiple of 16 elements.  probe int32 [nq x nprobe].  k <= 128, nlist <= 8192 (ivf_search_grouped_ok).
	_skip_gemm: measurement only (bench.py times the call with and without its tile launch; the results are then meaningless)."""
	_dev(lists, offsets, ids, Q, probe)
	lib = _lib.load()
	if lists.dtype != Q.dtype:
		raise ValueError("ivf_search_grouped: lists and queries must have the same dtype")
	nq_all, dp = Q.shape
	probe = probe.to(torch.int32).contiguous()
	nprobe, nlist = probe.shape[1], sizes_host.shape[0]
	lmax = max(int(sizes_host.max()), 1)
	k_eff = min(k, nprobe * lmax)
	pitch = -(-max(nprobe * lmax, k_eff) // 8) * 8                 # any row fits: nprobe lists of at most lmax vectors

	def run(q0, q1, ov, oi):
		nq, Qc, pr = q1 - q0, Q[q0:q1], probe[q0:q1]
		T = int(lib.anncur_ivf_search_tile(_dt(lists), dp, _ld(lists), _ld(Qc), nq))
		max_tiles = 0 if _skip_gemm else _ivf_max_tiles(nq * nprobe, sizes_host, T)
		S = _ScoreScratch.get(nq * pitch, Q.device)
		nbytes = lib.anncur_ivf_search_workspace_bytes(nq, nprobe, nlist, k_eff, max_tiles)
		ws = _ByteScratch.get(nbytes, Q.device)
		check(lib.anncur_ivf_search_grouped(_p(lists), _dt(lists), _ld(lists), dp, _p(offsets), _p(ids), nlist, _p(Qc), _ld(Qc), nq, _p(pr), nprobe, k_eff, max_tiles,
											_p(S), pitch, _p(ws), nbytes, _p(ov), _p(oi), _stream()), "ivf_search_grouped")

	step = max(64, min(nq_all, max_bytes // (pitch * 4), ((1 << 32) - 1) // pitch))
	return _ivf_chunked(nq_all, step, k, k_eff, Q.device, run)


@_on_device
def copy_to_mapped_host(src, pinned_host):
	"""Device kernel copy of `src` (CUDA tensor) into a PINNED host tensor (mapped into the device address space by the HIP
	runtime): graph-capturable, no copy engine.  The caller synchronises (event) before reading `pinned_host`.
	A copy of bytes: the two tensors need the same byte count, not the same dtype or shape; exactly those bytes of `pinned_host` are written
	(it may be a 16-byte-aligned contiguous view of a larger pinned tensor), `src` is not; zero bytes launch nothing."""
	if pinned_host.is_cuda or not pinned_host.is_pinned() or not pinned_host.is_contiguous():
		raise ValueError("copy_to_mapped_host needs a contiguous pinned host tensor")
	_dev(src)
	src = src.contiguous()
	nbytes = src.numel() * src.element_size()
	if nbytes != pinned_host.numel() * pinned_host.element_size():
		raise ValueError("size mismatch")
	check(_lib.load().anncur_copy_bytes(_p(src), ctypes.c_void_p(pinned_host.data_ptr()), nbytes, _stream()), "copy_bytes")
