"""anncur_amd/pinv.py's fp64 route restated in plain fp64 numpy -- the power iteration of pinv._spectral_norm_sq and the Newton-Schulz loop of
pinv.pinv_newton_schulz_f64, statement by statement: same start vector, same Gram matrix and power-of-two scale, same number of squarings
(read from pinv.py, not copied), same start scale min(1.1 s2, ||W||_F^2), same stopping rule -- and the spectrum families that the estimator and the gate of
pinv_backend="auto" are tested on.  A helper module, not a test: tests/test_cpu_pinv_reference.py holds the restatement against LAPACK and
records what the estimator does on the families, tests/test_gpu_pinv_gate.py and tests/test_gpu_pinv_newton_schulz.py hold the device against
both.  Only the sums differ from the device: numpy adds in its own order, the kernels in theirs (relative 1e-15 per sum)."""
import functools
import inspect
import math

import numpy as np

from anncur_amd import pinv as _pinv_module

POWER_SQUARINGS = inspect.signature(_pinv_module._spectral_norm_sq).parameters["squarings"].default   # what pinv.py runs (pinv.POWER_SQUARINGS)
POWER_STEPS = 2 ** POWER_SQUARINGS                                                                     # ... in single power steps
PARENT_POWER_STEPS = 8                                                                                 # what it ran before the gate was made sound


# ------------------------------------------------------------------ the restatement
def power_start(n):
	v = np.full((n, 1), 1.0 / n)
	v[::2] *= 1.5
	return v


def spectral_norm_sq(M, squarings=None):
	"""pinv._spectral_norm_sq: the Gram matrix of the short side, divided by a power of two above ||M||_F^2, squared `squarings` times and
	applied to the start vector; the Rayleigh quotient of that vector on M itself."""
	squarings = POWER_SQUARINGS if squarings is None else squarings
	M = np.asarray(M, dtype=np.float64)
	m, n = M.shape
	f2 = float((M * M).sum())
	if not (0.0 < f2 < float("inf")):
		return 0.0
	A = M if m <= n else M.T
	G = 2.0 ** -math.frexp(f2)[1] * (A @ A.T)
	for _ in range(squarings):
		G = G @ G
	v = G @ power_start(min(m, n))
	t = A.T @ v
	num, den = float((t * t).sum()), float((v * v).sum())
	return num / den if den > 0 else 0.0


def spectral_norm_sq_single_steps(M, steps=PARENT_POWER_STEPS):
	"""The estimator as it stood before: `steps` single steps v <- M^T M v / ||M^T M v||^2 from the start vector of length n, then the
	Rayleigh quotient ||M v||^2 / ||v||^2.  Kept to record what 8 of them did on the spectrum families."""
	M = np.asarray(M, dtype=np.float64)
	v = power_start(M.shape[1])
	with np.errstate(invalid="ignore", divide="ignore"):
		for _ in range(steps):
			u = M.T @ (M @ v)
			v = (1.0 * u) / float((u * u).sum())             # anncur_convert_f64's order: (alpha * src) / divide_by[0]
	t = M @ v
	num, den = float((t * t).sum()), float((v * v).sum())
	return num / den if den > 0 else 0.0


def newton_schulz_f64(W, max_iters=64, check_from=4, rtol=1e-10, squarings=None):
	"""pinv.pinv_newton_schulz_f64(W, return_info=True): W fp32 (or any array of fp32 values) -> (X fp32 [n x m], info)."""
	Wd = np.asarray(W).astype(np.float64)
	m, n = Wd.shape
	w2 = float((Wd * Wd).sum())
	s2 = spectral_norm_sq(Wd, squarings)
	if not (s2 > 0.0):
		s2 = w2
	scale = min(1.1 * s2, w2) if w2 > 0 else 1.0
	X = (1.0 * Wd.T) / scale
	tall = m >= n
	its, final = 0, False
	for it in range(max_iters):
		Xn = 2.0 * X - (X @ Wd) @ X if tall else 2.0 * X - X @ (Wd @ X)
		X, Xn = Xn, X
		its = it + 1
		if final:
			break
		if it >= check_from and (it - check_from) % 2 == 0:
			d2, x2 = float(((X - Xn) ** 2).sum()), float((X * X).sum())
			if not (x2 > 0.0) or not (x2 < 1e300) or d2 <= (rtol * rtol) * x2:
				final = x2 < 1e300
				if not final:
					break
	x2 = float((X * X).sum())
	xs2 = spectral_norm_sq(X, squarings) if final else float("inf")
	return X.astype(np.float32), {"iterations": its, "cond_F": (w2 * x2) ** 0.5, "cond_2": (s2 * xs2) ** 0.5, "converged": final}


# ------------------------------------------------------------------ the spectrum families
SHAPES = ((400, 160), (512, 256), (256, 512), (2048, 1024))     # all outside "auto"'s near-square shortcut: min <= 0.9 max
CONDS = (300.0, 700.0, 1050.0)
SEEDS = (0, 1, 2)
CLUSTER_R = (0.8, 0.85, 0.9, 0.96)
FAMILIES = ("power", "geometric", "flat1") + tuple(f"cluster{r}" for r in CLUSTER_R)


def spectrum(family, g, cond):
	"""g singular values, descending from 1 to 1 / cond."""
	j = np.arange(1, g + 1, dtype=np.float64)
	if family == "power":
		return j ** (-np.log(cond) / np.log(g))
	if family == "geometric":
		return cond ** (-(j - 1) / (g - 1))
	if family == "flat1":
		s = np.ones(g)
		s[-1] = 1.0 / cond
		return s
	if family.startswith("cluster"):                            # sigma_1 = 1, a cluster at r right below it, a second one above sigma_min = 1 / cond
		r = float(family[len("cluster"):])
		s = np.full(g, 1.0 / (cond * r))
		s[:g // 2] = r
		s[0], s[-1] = 1.0, 1.0 / cond
		return s
	raise ValueError(family)


@functools.lru_cache(maxsize=4)
def orthogonal_factors(m, n, seed):
	"""(U [m x g], V [n x g]) with orthonormal columns from a seeded Gaussian; shared by every family and cond of one (shape, seed)."""
	g = min(m, n)
	rng = np.random.default_rng([seed, m, n])
	U = np.linalg.qr(rng.standard_normal((m, g)))[0]
	V = np.linalg.qr(rng.standard_normal((n, g)))[0]
	U.setflags(write=False)
	V.setflags(write=False)
	return U, V


def members(shapes=SHAPES, conds=CONDS, seeds=SEEDS, families=FAMILIES):
	"""Every (family, (m, n), cond, seed), ordered so that consecutive members share their orthogonal factors."""
	return [(f, s, c, seed) for s in shapes for seed in seeds for f in families for c in conds]


def member_id(member):
	f, (m, n), c, seed = member
	return f"{f}-{m}x{n}-cond{c:g}-seed{seed}"


def build_member(member, with_pinv=False):
	"""-> (W fp32 [m x n] = U diag(sigma) V^T rounded once, the singular values of THAT fp32 matrix by LAPACK in fp64, descending
	[, its fp64 pseudo-inverse out of the same decomposition])."""
	family, (m, n), cond, seed = member
	U, V = orthogonal_factors(m, n, seed)
	W = ((U * spectrum(family, min(m, n), cond)) @ V.T).astype(np.float32)
	if not with_pinv:
		return W, np.linalg.svd(W.astype(np.float64), compute_uv=False)
	Us, S, Vt = np.linalg.svd(W.astype(np.float64), full_matrices=False)
	return W, S, (Vt.T / S) @ Us.T


def soundness(cond_true, smax2, s2, cond_2, safety):
	"""The three conditions that make the gate of pinv_backend="auto" sound, as a dict of booleans: the estimates are lower bounds (a Rayleigh
	quotient exceeds sigma_max^2 by rounding only: 1e-9 relative is ample in fp64), cond_2 is at most `safety` (cur.AUTO_COND_SAFETY) short, and
	one estimate of sigma_max^2 at most safety^2 short."""
	return {"cond_2 <= true": cond_2 <= cond_true * (1 + 1e-9),
			"true <= safety * cond_2": cond_true <= safety * cond_2,
			"s2 <= smax2": s2 <= smax2 * (1 + 1e-9),
			"smax2 <= safety^2 * s2": smax2 <= safety * safety * s2}
