"""The two Newton-Schulz iterations of anncur_amd/pinv.py on the device.

fp64 route (pinv_newton_schulz_f64, pinv_backend "device" / "auto"):
  * exact data -- W = H64[:, :48] diag(2^-(j mod 7)) (the block of tests/test_gpu_svd.py) and W^T, fp32 and bf16, fed as an interior view with a
    padded pitch: the pseudo-inverse diag(1/d) H^T / 64 is made of powers of two, the fp64 iterate ends within 1e-13 of it whatever the order of
    the kernels' sums, so the ONE rounding to fp32 must land on it bit for bit (a second rounding, or a result taken one step early, would not);
  * power-of-two equivariance -- pinv(2^k W) = 2^-k pinv(W) bit for bit, with equal iteration counts and an equal cond_2: every operation of
    the route scales exactly, an absolute constant hiding in a stopping rule or a start scale would break it.  The block is 96 x 40 so that
    no sum that feeds the result has more than two non-zero partial sums (they are combined by atomic adds, in no fixed order);
  * bf16 input against the fp32 input of the same values, bit for bit;
  * degenerate blocks: rank-deficient, all-zero, 1 x 1, single column / row, empty.
fp32 route (pinv_newton_schulz, "device32"): rho = ||X - X_ref||_F / ||X_ref||_F / (cond_2 2^-24) against fp64 LAPACK on the well-conditioned
  blocks of tests/test_gpu_cur.py and the Hadamard block, held to C32.  C32 was NOT chosen in advance: rho was measured on an MI355X over
  those inputs (the figures are in test_f32_route_against_fp64_lapack's docstring and DESIGN 4.5, and printed by every run) and C32 is 8 x the
  largest, rounded up to a power of two: 16.  The condition C32 <= 64 (above it the docstring's "cond * 6e-8" would be wrong) holds.  Two calls give equal bits -- which they did not while the
  route's two sums of squares were combined by atomic adds: ops.sumsq now adds in a fixed order (test_sumsq_adds_in_a_fixed_order).
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinv_numpy as P  # noqa: E402

pytestmark = pytest.mark.gpu

C32 = 16.0          # 8 x the largest measured rho (1.754, the 300 x 120 block: DESIGN 4.5) = 14.0, rounded up to a power of two
EPS32 = 2.0 ** -24
D48 = 2.0 ** -(np.arange(48) % 7)


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def hadamard(n):
	H = np.ones((1, 1))
	while H.shape[0] < n:
		H = np.block([[H, H], [H, -H]])
	return H


def _bits(t):
	return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _padded(W, dtype=torch.float32):
	"""Host array -> device view of it with a padded row pitch, the pad NaN."""
	rows, cols = W.shape
	big = torch.full((rows + 2, cols + 5), float("nan"), dtype=dtype, device="cuda")
	big[1:rows + 1, 2:cols + 2] = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).cuda().to(dtype)
	return big[1:rows + 1, 2:cols + 2]


def _hadamard_block(transposed):
	W, X = hadamard(64)[:, :48] * D48, (hadamard(64)[:, :48] / D48).T / 64.0
	return (W.T, X.T) if transposed else (W, X)


# ------------------------------------------------------------------ fp64 route: exact data
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
def test_f64_route_exact_hadamard_block_bit_for_bit(ops, dtype, transposed):
	from anncur_amd import pinv
	W, X_want = _hadamard_block(transposed)
	Wd = _padded(W, dtype)
	assert np.array_equal(Wd.float().cpu().numpy().astype(np.float64), W)         # (exact in bf16 too)
	X, info = pinv.pinv_newton_schulz_f64(Wd, return_info=True)
	assert info["converged"] and X.dtype == torch.float32 and tuple(X.shape) == X_want.shape
	assert np.array_equal(_bits(X), np.ascontiguousarray(X_want, dtype=np.float32).view(np.uint32))
	X_host, info_host = P.newton_schulz_f64(W.astype(np.float32))                  # the restatement: the same matrix after the same 20 steps
	assert info_host["iterations"] == 20 and info["iterations"] == 20
	assert np.array_equal(_bits(X), X_host.view(np.uint32))
	assert info["cond_2"] == pytest.approx(64.0, rel=1e-6) and info["cond_2"] <= 64.0 * (1 + 1e-9)


# ------------------------------------------------------------------ fp64 route: scaling by a power of two, bf16 input
@functools.lru_cache(maxsize=None)
def _generic_96x40():
	W = np.random.default_rng(9640).standard_normal((96, 40)).astype(np.float32)
	W.setflags(write=False)
	return W


def test_f64_route_power_of_two_equivariance(ops):
	from anncur_amd import pinv
	W = _generic_96x40()
	X, info = pinv.pinv_newton_schulz_f64(torch.tensor(W).cuda(), return_info=True)
	assert info["converged"]
	for k in (-20, 20):
		Wk = W * np.float32(2.0 ** k)
		assert np.array_equal(Wk.astype(np.float64), W.astype(np.float64) * 2.0 ** k)      # (the scaling itself is exact)
		Xk, ik = pinv.pinv_newton_schulz_f64(torch.from_numpy(Wk).cuda(), return_info=True)
		assert ik["converged"] and ik["iterations"] == info["iterations"]
		assert np.array_equal(_bits(Xk), _bits(X * 2.0 ** -k))
		assert ik["cond_2"] == info["cond_2"]                                           # equal bits: == on two finite floats


def test_f64_route_bf16_input_equals_the_fp32_input_of_the_same_values(ops):
	from anncur_amd import pinv
	Wb = torch.tensor(_generic_96x40()).bfloat16()
	Xb, ib = pinv.pinv_newton_schulz_f64(_padded(Wb.float().numpy(), torch.bfloat16), return_info=True)
	Xf, i_f = pinv.pinv_newton_schulz_f64(Wb.float().cuda(), return_info=True)
	assert ib["converged"] and np.array_equal(_bits(Xb), _bits(Xf))
	assert ib["iterations"] == i_f["iterations"] and ib["cond_2"] == i_f["cond_2"]


# ------------------------------------------------------------------ fp64 route: degenerate blocks
@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
def test_f64_route_rank_deficient_block(ops, transposed):
	"""tests/test_gpu_svd.py's block: 40 x 12 with a zero column and a duplicated one.  Reference: numpy.linalg.pinv in fp64 of the same fp32
	values at rcond 1e-10.  Bound: 2^-22 ||X_ref||_F -- the one fp32 rounding gives <= 2^-24 per element, the restatement shows 2.5e-8."""
	from anncur_amd import pinv
	W = np.random.default_rng(11).standard_normal((40, 12)).astype(np.float32)
	W[:, 7] = W[:, 3]
	W[:, 5] = 0.0
	X_ref = np.linalg.pinv(W.astype(np.float64), rcond=1e-10)
	if transposed:
		W, X_ref = np.ascontiguousarray(W.T), X_ref.T
	X, info = pinv.pinv_newton_schulz_f64(torch.from_numpy(W).cuda(), return_info=True)
	Xh = X.cpu().numpy().astype(np.float64)
	assert info["converged"] and np.isfinite(Xh).all(), info
	err = np.linalg.norm(Xh - X_ref) / np.linalg.norm(X_ref)
	print(f"rank-deficient {W.shape[0]} x {W.shape[1]}: {info['iterations']} iterations, ||X - X_ref||_F / ||X_ref||_F = {err:.3e} (bound {2.0 ** -22:.3e})")
	assert err <= 2.0 ** -22


def test_f64_route_zero_block(ops):
	from anncur_amd import cur, pinv
	Z = torch.zeros(5, 3, device="cuda")
	X, info = pinv.pinv_newton_schulz_f64(Z, return_info=True)
	assert info["converged"] and info["cond_2"] == 0
	assert tuple(X.shape) == (3, 5) and X.dtype == torch.float32 and not _bits(X).any()      # +0.0 everywhere
	U = cur._pinv(Z.cpu(), torch.device("cuda"), "auto")
	assert tuple(U.shape) == (3, 5) and not _bits(U).any()


def test_f64_route_one_by_one_and_single_vectors(ops):
	from anncur_amd import pinv
	X, info = pinv.pinv_newton_schulz_f64(torch.tensor([[3.0]], device="cuda"), return_info=True)
	assert info["converged"] and _bits(X).tolist() == [[int(np.float32(1.0 / 3.0).view(np.uint32))]]
	w = np.arange(1.0, 8.0, dtype=np.float32).reshape(7, 1)
	want = (w.astype(np.float64).T / 140.0).astype(np.float32)                    # w^T / ||w||^2, correctly rounded (1 + 4 + ... + 49 = 140)
	for M, R in ((w, want), (np.ascontiguousarray(w.T), np.ascontiguousarray(want.T))):
		X, info = pinv.pinv_newton_schulz_f64(torch.from_numpy(M).cuda(), return_info=True)
		assert info["converged"] and tuple(X.shape) == R.shape
		assert np.array_equal(_bits(X), R.view(np.uint32))


@pytest.mark.parametrize("backend", ["auto", "device"])
@pytest.mark.parametrize("shape", [(0, 4), (4, 0), (0, 0)])
def test_empty_blocks_through_cur_pinv(ops, shape, backend):
	from anncur_amd import cur
	U = cur._pinv(torch.zeros(shape), torch.device("cuda"), backend)
	assert tuple(U.shape) == shape[::-1] and U.dtype == torch.float32 and U.is_cuda and not U.any()


# ------------------------------------------------------------------ fp32 route
F32_CASES = {"512x256": (512, 256, 64, 0.05), "256x512": (256, 512, 64, 0.05), "300x120": (300, 120, 300, 1.0), "2048x1024": (2048, 1024, 64, 0.05),
			 "hadamard": None}


@functools.lru_cache(maxsize=None)
def _f32_case(name):
	"""-> (W fp32, fp64 LAPACK pseudo-inverse of the same values, cond_2): computed once, shared, never written to."""
	if F32_CASES[name] is None:
		W = _hadamard_block(False)[0].astype(np.float32)
	else:
		m, n, rank, noise = F32_CASES[name]                                       # the blocks of test_device_pinv_f64_is_the_exact_pseudo_inverse
		g = torch.Generator().manual_seed(m + n)
		r = min(rank, m, n)
		W = (torch.randn(m, r, generator=g) @ torch.randn(r, n, generator=g) / rank ** 0.5 + noise * torch.randn(m, n, generator=g)).numpy()
	U, S, Vt = np.linalg.svd(W.astype(np.float64), full_matrices=False)
	X_ref = (Vt.T / S) @ U.T
	for a in (W, X_ref):
		a.setflags(write=False)
	return W, X_ref, float(S[0] / S[-1])


@pytest.mark.parametrize("name", list(F32_CASES))
def test_f32_route_against_fp64_lapack(ops, name):
	"""Measured on an MI355X (rho, then the Moore-Penrose residual ||W X W - W||_F / ||W||_F on the same scale cond_2 2^-24):
	512 x 256 (cond_2 195.7) 0.427 / 0.537; 256 x 512 (204.7) 0.404 / 0.501; 300 x 120 (4.5) 1.754 / 1.010; 2048 x 1024 (338.5) 0.522 / 0.698;
	Hadamard 64 x 48 (64) 0.037 / 0.017.  The numpy fp32 restatement of the issue gave 0.4 .. 1.7.  C32 = 16 covers both figures."""
	from anncur_amd import pinv
	W, X_ref, cond = _f32_case(name)
	Wg = torch.tensor(W).cuda()
	X = pinv.pinv_newton_schulz(Wg)
	assert X.dtype == torch.float32 and tuple(X.shape) == X_ref.shape
	Xh = X.cpu().numpy().astype(np.float64)
	W64 = W.astype(np.float64)
	scale = cond * EPS32
	rho = np.linalg.norm(Xh - X_ref) / np.linalg.norm(X_ref) / scale
	mp = np.linalg.norm(W64 @ Xh @ W64 - W64) / np.linalg.norm(W64) / scale
	print(f"fp32 Newton-Schulz {name}: cond_2 {cond:.1f}, rho = {rho:.3f}, ||W X W - W||_F / ||W||_F / (cond_2 2^-24) = {mp:.3f}; allowed {C32:g}")
	assert np.isfinite(Xh).all() and rho <= C32 and mp <= C32
	again = pinv.pinv_newton_schulz(Wg)
	assert np.array_equal(_bits(again), _bits(X)), "two calls on the same block gave different bits"


def test_sumsq_adds_in_a_fixed_order(ops):
	"""What the equal bits above rest on: the fp32 route scales X_0 by ops.sumsq(W) and stops on ops.sumsq(X), so a sum whose last bit moved
	from call to call (anncur_sumsq: atomic adds in the order the waves finish) gave every call other bits.  The ordered sum
	(anncur_sumsq_ordered) gives one value, within the rounding of any order of its n terms of the fp64 sum; both routes stay exact on integers;
	shapes on both sides of one workgroup's 2048 elements and past the 1024 workgroups."""
	for rows, cols, pad in ((1, 1, 0), (3, 700, 5), (2049, 1031, 1), (1500, 2048, 3)):
		g = torch.Generator().manual_seed(rows + cols)
		buf = torch.full((rows + 1, cols + pad), float("nan"), device="cuda")
		A = buf[:rows, :cols]
		A.copy_(torch.randn(rows, cols, generator=g).cuda())
		first = ops.sumsq(A)
		want = float((A.double() ** 2).sum().item())
		# no term passes more than 34 roundings: its square, <= 12 adds in its thread, 6 shuffles, 3 waves, <= 4 partials per thread, 8 tree levels
		assert abs(float(first.item()) - want) <= 40 * EPS32 * want
		out = torch.full((1,), float("nan"), device="cuda")
		for _ in range(10):
			assert ops.sumsq(A, out=out).data_ptr() == out.data_ptr() and _bits(out) == _bits(first)
		A.copy_(torch.randint(-2, 3, (rows, cols), generator=g).float().cuda())
		exact = float((A.double() ** 2).sum().item())
		assert float(ops.sumsq(A).item()) == exact and float(ops.sumsq(A, ordered=False).item()) == exact
	Z = torch.zeros(0, 7, device="cuda")
	assert float(ops.sumsq(Z).item()) == 0.0 and float(ops.sumsq(Z, ordered=False).item()) == 0.0


@pytest.mark.parametrize("name", list(F32_CASES))
def test_cur_device32_backend_is_the_fp32_route(ops, name):
	from anncur_amd import pinv
	from anncur_amd.cur import CURApprox
	W = torch.tensor(_f32_case(name)[0])
	m, n = W.shape
	c = CURApprox(rows=W, cols=W, row_idxs=list(range(m)), col_idxs=list(range(n)), approx_preference="rows", pinv_backend="device32")
	assert np.array_equal(_bits(c.U), _bits(pinv.pinv_newton_schulz(W.cuda())))
