"""tests/pinv_numpy.py (the host statement of pinv.py's fp64 route that the GPU tests compare with) against LAPACK and hand-worked blocks,
and what its power iteration does on the spectrum families of the gate tests: every member is built as the tests say (fp32 rounding moves
cond_2 by < 2 %), the 8 steps of the estimator before the gate was made sound break the soundness conditions on a named member -- the proof
that tests/test_gpu_pinv_gate.py bites -- and the estimator pinv.py runs now meets them on every member.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinv_numpy as P  # noqa: E402

from anncur_amd import cur, pinv  # noqa: E402

SAFETY = cur.AUTO_COND_SAFETY


def hadamard(n):
	H = np.ones((1, 1))
	while H.shape[0] < n:
		H = np.block([[H, H], [H, -H]])
	return H


def test_step_count_is_read_from_pinv_py():
	assert P.POWER_SQUARINGS == pinv.POWER_SQUARINGS and P.POWER_STEPS == 2 ** pinv.POWER_SQUARINGS > P.PARENT_POWER_STEPS
	assert cur.AUTO_COND_LIMIT / SAFETY == 800.0          # the gate tests' 700 -> device and 1050 -> host rest on this


# ------------------------------------------------------------------ the restatement against LAPACK and exact blocks
@pytest.mark.parametrize("shape", [(96, 40), (40, 96), (33, 33), (5, 1)])
def test_restatement_is_the_pseudo_inverse(shape):
	W = np.random.default_rng(shape[0] * 100 + shape[1]).standard_normal(shape).astype(np.float32)
	X, info = P.newton_schulz_f64(W)
	S = np.linalg.svd(W.astype(np.float64), compute_uv=False)
	ref = np.linalg.pinv(W.astype(np.float64))
	assert info["converged"] and X.dtype == np.float32 and X.shape == shape[::-1]
	assert np.linalg.norm(X - ref) <= 2.0 ** -24 * np.linalg.norm(ref)          # one fp32 rounding per element
	c = S[0] / S[-1]
	assert c / SAFETY <= info["cond_2"] <= c * (1 + 1e-9)
	assert info["cond_F"] == pytest.approx(np.linalg.norm(S) * np.linalg.norm(1 / S), rel=1e-9)


@pytest.mark.parametrize("transposed", [False, True])
def test_restatement_is_exact_on_the_hadamard_block(transposed):
	"""W = H64[:, :48] diag(2^-(j mod 7)): the pseudo-inverse diag(1/d) H^T / 64 is made of powers of two, the fp64 iterate ends within 1e-13
	of it in any order of the sums, and the one rounding to fp32 lands on it -- in 20 steps, the last of them after the stopping rule fired."""
	d = 2.0 ** -(np.arange(48) % 7)
	W, want = hadamard(64)[:, :48] * d, (hadamard(64)[:, :48] / d).T / 64.0
	if transposed:
		W, want = W.T, want.T
	X, info = P.newton_schulz_f64(W.astype(np.float32))
	assert info["converged"] and info["iterations"] == 20
	assert np.array_equal(X.view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_restatement_on_degenerate_blocks():
	W = np.random.default_rng(11).standard_normal((40, 12)).astype(np.float32)
	W[:, 7] = W[:, 3]
	W[:, 5] = 0.0
	ref = np.linalg.pinv(W.astype(np.float64), rcond=1e-10)
	for M, R in ((W, ref), (W.T, ref.T)):
		X, info = P.newton_schulz_f64(M)
		rel = np.linalg.norm(X - R) / np.linalg.norm(R)
		assert info["converged"] and np.isfinite(X).all() and rel <= 2.0 ** -22 / 8, rel     # (2.5e-8: the GPU test's bound has 8x over this)
	X, info = P.newton_schulz_f64(np.zeros((5, 3), dtype=np.float32))
	assert info["converged"] and info["cond_2"] == 0.0 and X.shape == (3, 5) and not X.any()
	X, info = P.newton_schulz_f64(np.array([[3.0]], dtype=np.float32))
	assert info["converged"] and X[0, 0] == np.float32(1.0 / 3.0)
	w = np.arange(1.0, 8.0, dtype=np.float32).reshape(7, 1)
	want = (w.astype(np.float64).T / 140.0).astype(np.float32)                            # correctly rounded w^T / ||w||^2
	for M, R in ((w, want), (w.T, want.T)):
		X, info = P.newton_schulz_f64(M)
		assert info["converged"] and np.array_equal(X.view(np.uint32), np.ascontiguousarray(R).view(np.uint32))


def test_power_of_two_scaling_is_exact_in_the_restatement():
	W = np.random.default_rng(9640).standard_normal((96, 40)).astype(np.float32)
	X, info = P.newton_schulz_f64(W)
	for k in (-20, 20):
		Xk, ik = P.newton_schulz_f64(W * np.float32(2.0 ** k))
		assert np.array_equal(Xk.view(np.uint32), (X * np.float32(2.0 ** -k)).view(np.uint32))
		assert ik["iterations"] == info["iterations"] and ik["cond_2"] == info["cond_2"]


# ------------------------------------------------------------------ the estimator on the spectrum families
# The member on which the parent's 8 steps break `true <= AUTO_COND_SAFETY * cond_2`: true / estimate = 1.33 there (1.28 on
# cluster0.8-256x512-cond1050-seed1; both found by running this file's loop over the set with 8 steps).
BROKEN_AT_8 = ("cluster0.85", (512, 256), 300.0, 1)


def test_family_set_is_what_the_gate_tests_say():
	ms = P.members()
	assert len(ms) == len(set(ms)) == 7 * 4 * 3 * 3 and BROKEN_AT_8 in ms
	assert all(min(s) <= cur.AUTO_SQUARE_RATIO * max(s) for s in P.SHAPES)            # outside "auto"'s near-square shortcut
	for f in P.FAMILIES:
		s = P.spectrum(f, 160, 700.0)
		assert s[0] == 1.0 and s[-1] == pytest.approx(1 / 700.0, rel=1e-12) and np.all(s[:-1] >= s[1:])
	s = P.spectrum("cluster0.8", 256, 900.0)                                            # sigma_1 = 1, sigma_2..128 = r, the rest 1 / (cond r), sigma_min
	assert s[0] == 1 and np.all(s[1:128] == 0.8) and np.all(s[128:255] == 1 / (900.0 * 0.8)) and s[255] == 1 / 900.0


def _estimates(member, estimator):
	W, S, X = P.build_member(member, with_pinv=True)
	assert abs(S[0] / S[-1] / member[2] - 1.0) < 0.02, "fp32 rounding moved cond_2 by 2 % or more"
	s2 = estimator(W.astype(np.float64))
	# the estimate on X: the fp64 pseudo-inverse by LAPACK stands in for the converged Newton-Schulz iterate -- the two differ by 1e-10 ||X||
	# (the stopping rule's rtol), which moves a Rayleigh quotient by 2e-10 relative, inside the 1e-9 of the conditions
	xs2 = estimator(X)
	return S[0] / S[-1], S[0] ** 2, s2, (s2 * xs2) ** 0.5


def test_parent_estimator_breaks_the_soundness_condition():
	"""(a) 8 steps, as pinv._spectral_norm_sq ran them before: the cond_2 estimate is more than AUTO_COND_SAFETY short on BROKEN_AT_8."""
	cond_true, smax2, s2, cond_2 = _estimates(BROKEN_AT_8, P.spectral_norm_sq_single_steps)
	ok = P.soundness(cond_true, smax2, s2, cond_2, SAFETY)
	assert not ok["true <= safety * cond_2"] and cond_true / cond_2 > 1.3, (cond_true, cond_2)
	assert ok["cond_2 <= true"] and ok["s2 <= smax2"]                               # (short, never over: it is a lower bound)


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_estimator_is_sound_on_every_member(shape, seed):
	"""(b) the estimator pinv.py runs now (the Gram matrix squared pinv.POWER_SQUARINGS times) meets all the conditions on all 252 members (21 per case)."""
	worst = {}
	for member in P.members(shapes=(shape,), seeds=(seed,)):
		cond_true, smax2, s2, cond_2 = _estimates(member, P.spectral_norm_sq)
		ok = P.soundness(cond_true, smax2, s2, cond_2, SAFETY)
		assert all(ok.values()), (P.member_id(member), ok, cond_true, cond_2, smax2 / s2)
		w = worst.setdefault(member[0], [0.0, 0.0])
		w[0], w[1] = max(w[0], cond_true / cond_2), max(w[1], smax2 / s2)
	print(f"{shape[0]} x {shape[1]} seed {seed}, {P.POWER_STEPS} steps, worst true / cond_2 (sigma_max^2 / s2): " + ", ".join(f"{f} {a:.4f} ({b:.4f})" for f, (a, b) in worst.items()))
