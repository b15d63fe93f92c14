"""Moore-Penrose pseudo-inverse on the GPU by Newton-Schulz iteration,

    X_0 = W^T / ||W||_F^2 ,   X_{k+1} = 2 X_k - X_k W X_k ,

which converges (quadratically, once the smallest eigenvalue of X_k W leaves 0) to W^+ for ANY W, needs nothing but GEMMs --
here the fp32-MFMA kernel of the C ABI -- and no host round trip except an occasional 2-float convergence check.
It is the on-device alternative to the reference's host call ``numpy.linalg.pinv`` (eval/matrix_approx_zeshel.py:47,49; LAPACK
SVD, rcond 1e-15).  Two routes live here: the fp64 iteration (pinv_newton_schulz_f64: the exact pseudo-inverse of the fp32 block,
rounded once -- what cur.py's default backend "auto" runs while the block is well conditioned; only backend "numpy", the same
LAPACK call as the reference, makes U bit-identical) and round 1's fp32 iteration (pinv_newton_schulz, backend "device32":
accuracy ~ cond(W) * 6e-8 like an fp32 SVD, singular values below ~1e-4 * sigma_max effectively truncated by the iteration cap).
The device routes matter for large anchor counts, where the host SVD dominates the index build (2048 x 1024: 1.4 s on the host, a
few ms here).  A third route, pinv_svd (backend "svd", opt-in), decomposes the block by Jacobi rotations in fp64 and is the only one
that can leave singular values below a cutoff out: no faster than the host call, but it truncates and reports the spectrum."""
import math

import torch

from . import ops


def pinv_newton_schulz(W, max_iters=80, check_every=4, rtol=1e-6):
	"""W: [m x n] fp32 / bf16 tensor on the GPU -> W^+ [n x m] fp32 on the GPU.  Equal inputs give equal bits: the GEMMs add in k order and
	the two sums the run depends on (the start scale, the stopping rule) are ops.sumsq's ordered ones."""
	if W.dtype != torch.float32:
		W = ops.convert(W, torch.float32)
	m, n = W.shape
	fro = ops.sumsq(W)
	X = torch.empty((n, m), dtype=torch.float32, device=W.device)
	ops.scale_copy(W.t(), X, 1.0, divide_by=fro)            # X_0 = W^T / ||W||_F^2  (||W||_2^2 <= ||W||_F^2: contraction)
	Xn = torch.empty_like(X)
	tall = m >= n                                            # iterate with the smaller Gram side
	P = torch.empty((n, n) if tall else (m, m), dtype=torch.float32, device=W.device)
	norms = torch.zeros(2, dtype=torch.float32, device=W.device)
	prev = None
	for it in range(max_iters):
		if tall:
			ops.gemm(X, W, out=P)                            # P = X W            [n x n]
			ops.gemm(P, X, out=Xn, alpha=-1.0, beta=2.0, cin=X)   # X' = 2 X - P X
		else:
			ops.gemm(W, X, out=P)                            # P = W X            [m x m]
			ops.gemm(X, P, out=Xn, alpha=-1.0, beta=2.0, cin=X)   # X' = 2 X - X P
		X, Xn = Xn, X
		if it >= 8 and (it % check_every) == 0:              # ||X_k||_F grows monotonically towards ||W^+||_F
			cur = float(ops.sumsq(X, out=norms[0:1]).item())
			if prev is not None and abs(cur - prev) <= rtol * cur:
				break
			prev = cur
	return X


POWER_SQUARINGS = 5   # _spectral_norm_sq applies G^(2^5) to its start vector: 32 power steps for the price of 5 small GEMMs


def _spectral_norm_sq(M, squarings=POWER_SQUARINGS):
	"""||M||_2^2 by power iteration on the Gram matrix of M's short side, G = A A^T [g x g] (A = M or M^T, g = min(m, n)): G is squared
	`squarings` times -- G^(2^k) in k GEMMs of g^3, where the same number of single steps took 2^(k+1) GEMVs over all of M, each a launch that
	fills a few workgroups -- then v = G^(2^k) v_0, and the result is the Rayleigh quotient ||A^T v||^2 / ||v||^2 on M itself.  Two host
	reads: ||M||_F^2 at the start, the quotient at the end.
	G is divided once by a power of two >= ||M||_F^2 >= sigma_max^2: its eigenvalues are then <= 1, the largest > 1 / (2 g), so 2^5 powers
	neither overflow nor lose the top direction ((2 g)^-32 >= 2^-672 for g <= 2^20), and being a power of two the scale changes no mantissa:
	the result is the same bits whichever one is taken, and scales exactly with a power-of-two multiple of M.
	The quotient of ANY v is a lower bound, so the result is never above sigma_max^2 except by rounding (1e-9 relative is ample); how far
	below depends on how much of v_0 lies along the top singular vector and on the gap under sigma_max.  What is held by test on the spectrum
	families of tests/pinv_numpy.py (power-law, geometric, flat, two clusters with sigma_2 / sigma_1 = 0.8 .. 0.96; up to 2048 x 1024,
	cond_2 300 .. 1050) is sigma_max^2 / 1.25^2 <= result <= sigma_max^2 (1 + 1e-9), and for cond_2, the root of two such estimates,
	cond_2 <= true <= 1.25 cond_2 (cur.AUTO_COND_SAFETY).  That serves both callers: X_0 = W^T / (1.1 s2) contracts while
	s2 > sigma_max^2 / 2.2.  A slowly converging quotient sits near sigma_2^2, so a cluster with (sigma_2 / sigma_1)^2 >= 0.8 is inside the
	factor at any step count; the steps are there for the clusters below that, which the 8 single steps this replaced did not leave (one
	estimate up to 1.55 short, cond_2 up to 1.33).  Nothing covers a v_0 that is orthogonal to the top singular vector to many digits.
	M: [m x n] fp64.  0.0 for a zero matrix and for one whose ||M||_F^2 is not finite."""
	m, n = M.shape
	if not M.is_contiguous():
		M = M.contiguous()
	nrm = torch.empty(2, dtype=torch.float64, device=M.device)
	f2 = float(ops.diff_sumsq_f64(M, out=nrm)[1].item())
	if not (0.0 < f2 < float("inf")):
		return 0.0
	A = M if m <= n else M.t()                               # [g x L]: the short side's vectors as rows
	g = min(m, n)
	G = ops.gemm_f64(A, A.t(), alpha=2.0 ** -math.frexp(f2)[1])   # (frexp: f2 = x 2^e with x in [0.5, 1), so 2^e > f2)
	B = torch.empty_like(G)
	for _ in range(squarings):
		ops.gemm_f64(G, G, out=B)
		G, B = B, G
	v0 = torch.full((g, 1), 1.0 / g, dtype=torch.float64, device=M.device)
	v0[::2] *= 1.5                                           # (not orthogonal to anything structured)
	v = ops.gemm_f64(G, v0)                                  # v = G^(2^k) v_0
	t = ops.gemm_f64(A.t(), v)                               # [L x 1]
	num = float(ops.diff_sumsq_f64(t, out=nrm)[1].item())
	den = float(ops.diff_sumsq_f64(v, out=nrm)[1].item())
	return num / den if den > 0 else 0.0


def pinv_newton_schulz_f64(W, max_iters=64, check_from=4, rtol=1e-10, return_info=False):
	"""Parity-grade pseudo-inverse: Newton-Schulz in DOUBLE precision on the fp64 matrix cores (anncur_gemm_f64), the result
	rounded to fp32 once.  W: [m x n] fp32 / bf16 on the GPU -> W^+ [n x m] fp32 on the GPU.

	X_0 = W^T / (1.1 sigma_max^2) with sigma_max from a power iteration on the Gram matrix (_spectral_norm_sq; iterations ~ 2 log2 cond(W) + 4 instead of
	+ log2 rank with the Frobenius scaling).  In fp64 the iteration resolves singular values down to ~2^-(iters/2) of the
	largest, i.e. it converges to the exact pseudo-inverse of the fp32 matrix W for any conditioning the fp32 SVD of
	numpy.linalg.pinv can resolve; what separates the two is then numpy's own fp32 round-off (~cond(W) * 6e-8).  Stops when
	||X_k+1 - X_k||_F <= rtol ||X_k||_F (checked every second iteration: one 16-byte D2H each), followed by one more
	(quadratically convergent) step.  64 iterations resolve cond(W) up to ~1e8: a block that has not converged by then is singular
	to fp32 precision (numpy then inverts singular values that are fp32 round-off, and so would this iteration, to different
	noise) -- info["converged"] is False and the caller (cur._pinv) hands such a block to the host's LAPACK call, as the reference
	does.
	info: iterations, converged, cond_2 = ||W||_2 ||W^+||_2 (both by _spectral_norm_sq, so a lower bound, at most 1.25 short on the
	families it is tested on: the caller's handle on how far numpy's fp32 SVD can be trusted), cond_F."""
	m, n = W.shape
	Wd = torch.empty((m, n), dtype=torch.float64, device=W.device)
	ops.convert_f64(W, Wd)
	norms = ops.diff_sumsq_f64(Wd)                          # [0, ||W||_F^2]
	s2 = _spectral_norm_sq(Wd)
	w2 = float(norms[1].item())
	if not (s2 > 0.0):
		s2 = w2
	scale = torch.full((1,), min(1.1 * s2, w2) if w2 > 0 else 1.0, dtype=torch.float64, device=W.device)   # (||W||_F^2 always contracts)
	X = torch.empty((n, m), dtype=torch.float64, device=W.device)
	ops.convert_f64(Wd.t(), X, 1.0, divide_by=scale)        # X_0 = W^T / (1.1 sigma_max^2)
	Xn = torch.empty_like(X)
	tall = m >= n
	P = torch.empty((n, n) if tall else (m, m), dtype=torch.float64, device=W.device)
	chk = torch.empty(2, dtype=torch.float64, device=W.device)
	its, final = 0, False
	for it in range(max_iters):
		if tall:
			ops.gemm_f64(X, Wd, out=P)                                  # P = X W   [n x n]
			ops.gemm_f64(P, X, out=Xn, alpha=-1.0, beta=2.0, cin=X)     # X' = 2 X - P X
		else:
			ops.gemm_f64(Wd, X, out=P)                                  # P = W X   [m x m]
			ops.gemm_f64(X, P, out=Xn, alpha=-1.0, beta=2.0, cin=X)     # X' = 2 X - X P
		X, Xn = Xn, X
		its = it + 1
		if final:
			break
		if it >= check_from and (it - check_from) % 2 == 0:
			d2, x2 = ops.diff_sumsq_f64(X, Xn, out=chk).tolist()
			if not (x2 > 0.0) or not (x2 < 1e300) or d2 <= (rtol * rtol) * x2:
				final = x2 < 1e300
				if not final:
					break
	out = torch.empty((n, m), dtype=torch.float32, device=W.device)
	ops.convert_f64(X, out)
	if return_info:
		x2 = float(ops.diff_sumsq_f64(X, out=chk)[1].item())
		xs2 = _spectral_norm_sq(X) if final else float("inf")
		return out, {"iterations": its, "cond_F": (w2 * x2) ** 0.5, "cond_2": (s2 * xs2) ** 0.5, "converged": final}
	return out


def pinv_svd(W, rcond=1e-15, return_info=False, max_sweeps=30):
	"""Truncated pseudo-inverse through the Jacobi SVD on the device (ops.svd_jacobi + ops.pinv_from_svd): the one device route
	with a cutoff; its sweep count barely depends on cond(W) (10-18 sweeps measured from cond 1e2 to 4e5), where Newton-Schulz needs
	~2 log2 cond(W) GEMM pairs -- which are still far cheaper at the sizes measured (DESIGN 4.5a has the table).  W: [m x n] fp32 / bf16 on the GPU -> W^+ [n x m] fp32 on the GPU: the singular values above
	rcond * sigma_max inverted (numpy.linalg.pinv's rule), the sum in fp64, one rounding.  1 <= min(m, n) <= 2048, max(m, n) <= 8192 and
	0 <= rcond < 1, else ValueError.
	info: singular_values (fp64 on the device, descending), rank (those kept), sweeps, converged (False: max_sweeps ran out, or a singular
	value is not finite; X is then what the unfinished iteration gives, and the caller -- cur._pinv -- hands the block to the host)."""
	rcond = ops._rcond_check(rcond, "pinv_svd")
	svd = ops.svd_jacobi(W, max_sweeps=max_sweeps)
	X, rank = ops.pinv_from_svd(svd, rcond)
	if return_info:
		return X, {"singular_values": svd.S, "rank": rank, "sweeps": svd.sweeps, "converged": svd.converged}
	return X
