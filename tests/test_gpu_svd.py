"""ops.svd_jacobi / ops.pinv_from_svd / pinv.pinv_svd (anncur_svd_*) on the device.

Exact data: W = H64[:, :48] diag(d), H64 the Sylvester Hadamard matrix, d_j = 2^-(j mod 7).  Every pair's h_i . h_j is a sum of +-d_i d_j
terms that cancel exactly in ANY order, so the first sweep rotates nothing (sweeps == 1), S = 8 d sorted and the pseudo-inverse
diag(1/d) H^T / 64 are powers of two times +-1: asserted for equality, bit for bit, for W and W^T, fp32 and bf16, a padded row pitch, a
workspace poisoned with 0xff and guard elements behind every output.
Generic data against numpy.linalg.svd in fp64 on the same fp32 values: the four error figures are held to C g 2^-53 sigma_max.  C was NOT
chosen in advance: the largest ratio error / (g 2^-53 sigma_max) over the ten shapes was measured on an MI355X (the figures are in DESIGN
4.5a and printed by every run of the test) and C is 8 times that, rounded up to a power of two -- the margin covers other seeds and LAPACK's
own error.  The issue's condition C <= 1024 (above it the iteration would not reach fp64 accuracy) holds.
The same two kinds of data above 256 vectors, where every loop over g takes more than one pass: the exact block at g = 600 (H_1024) and at the
limit g = 2048 (H_4096, S = 64 d), generic 300 x 320, 700 x 513 and 300 x 2100, a truncation among 300 singular values, and the fixed matrix
[[2, 1], [1, 2]] whose first rotation has zeta == 0.

Mutations tried on scratch builds when the tests above 256 vectors were written (each only drops work; every test this file had before PASSES on
both -- the largest g was 130):
  * svd_pair_kernel rotates only the first 256 entries of Vt's rows: generic 300 x 320, 700 x 513 and 300 x 2100 fail (V^T V - I or U^T U - I)
    and so do both truncations among 300 singular values (5 tests).  The exact blocks pass: nothing rotates on them.
  * svd_scale_cols_kernel counts the rank over its first pass only: the exact blocks at g = 600 (4 tests) and g = 2048 (2) fail, and the
    truncation at rank 271; the one at rank 152 passes, as it must (every kept value lies in the first pass).
Needs an MI355X."""
import functools
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32.0            # 8 x the largest measured ratio (2.604, V^T V - I of the 96 x 96 block: DESIGN 4.5a) = 20.8, rounded up to a power of two
EPS = 2.0 ** -53
SHAPES = [(1, 1), (1, 40), (2, 2), (5, 3), (33, 17), (64, 64), (96, 96), (96, 192), (192, 96), (257, 130), (300, 320), (700, 513)]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def hadamard(n):
	"""Sylvester's H_n as int8 (H_4096 is 16 MB this way); a product with a float64 array widens it."""
	H = np.ones((1, 1), dtype=np.int8)
	while H.shape[0] < n:
		H = np.block([[H, H], [H, -H]])
	return H


@functools.lru_cache(maxsize=None)
def generic(rows, cols):
	"""(W fp32, numpy's fp64 SVD of the same values): computed once, shared, never written to."""
	W = np.random.default_rng(1000 * rows + cols).standard_normal((rows, cols)).astype(np.float32)
	U, S, Vt = np.linalg.svd(W.astype(np.float64), full_matrices=False)
	for a in (W, U, S, Vt):
		a.setflags(write=False)
	return W, U, S, Vt


def ratios(W, S_ref, svd):
	"""The four figures of the generic test, each divided by g 2^-53 sigma_max (sigma_max = 1 for the two orthogonality terms)."""
	g = min(W.shape)
	U, S, V = svd.U.cpu().numpy(), svd.S.cpu().numpy(), svd.V.cpu().numpy()
	smax = S_ref[0]
	W64 = W.astype(np.float64)
	return {"S": np.abs(S - S_ref).max() / (g * EPS * smax),
			"UtU": np.abs(U.T @ U - np.eye(g)).max() / (g * EPS),
			"VtV": np.abs(V.T @ V - np.eye(g)).max() / (g * EPS),
			"USVt": np.abs((U * S) @ V.T - W64).max() / (g * EPS * smax)}


# ------------------------------------------------------------------ 1. exact data
def _guarded(shape, pitch, device, fill):
	"""A [shape] fp64 view with row pitch `pitch` inside a buffer filled with `fill`, 64 guard elements behind it -> (view, buffer)."""
	n = (shape[0] - 1) * pitch + shape[1] if len(shape) == 2 else shape[0]
	buf = torch.full((n + 64,), fill, dtype=torch.float64, device=device)
	view = buf[:n] if len(shape) == 1 else torch.as_strided(buf, shape, (pitch, 1))
	return view, buf


def _exact_hadamard_block(ops, n, g, dtype, transposed):
	"""W = H_n[:, :g] diag(d), d_j = 2^-(j mod 7), n a power of 4 (sqrt(n) a power of two): sweeps == 1 with zero rotations, S = sqrt(n) d sorted,
	the pseudo-inverse diag(1/d) H^T / n bit for bit, and the cutoff 2^-3.5 between two singular values."""
	dev = torch.device("cuda")
	root = int(round(n ** 0.5))
	assert root * root == n and root & (root - 1) == 0
	D = 2.0 ** -(np.arange(g) % 7)
	Hg = hadamard(n)[:, :g]
	W = Hg * D                                                           # n x g, every entry +-2^-k
	X_want = (Hg / D).T / float(n)                                        # g x n = diag(1/d) H^T / n
	if transposed:
		W, X_want = W.T, X_want.T
	rows, cols = W.shape
	big = torch.full((rows, cols + 5), float("nan"), dtype=dtype, device=dev)    # a padded row pitch, the pad poisoned
	big[:, :cols] = torch.from_numpy(W.astype(np.float32)).to(dev).to(dtype)
	Wd = big[:, :cols]
	assert np.array_equal(Wd.float().cpu().numpy().astype(np.float64), W)         # (exact in bf16 too)
	need = ops._lib.load().anncur_svd_workspace_bytes(rows, cols)
	wsbuf = torch.full((need + 512,), 0xff, dtype=torch.uint8, device=dev)       # every double of the workspace starts as a NaN
	off = (-wsbuf.data_ptr()) % 256
	ws = wsbuf[off:off + need]
	SENT = -777.25
	sigma, sbuf = _guarded((g,), 0, dev, SENT)
	U, ubuf = _guarded((rows, g), g + 3, dev, SENT)
	V, vbuf = _guarded((cols, g), g + 7, dev, SENT)
	ints = torch.full((2, 16), 12345, dtype=torch.int32, device=dev)
	rot, flag = ints[0, :1], ints[1, :1]
	_, _, _, sweeps, converged = ops.svd_jacobi_unsorted(Wd, workspace=ws, out=(sigma, U, V, rot, flag))
	torch.cuda.synchronize()
	assert sweeps == 1 and converged
	assert int(rot.item()) == 0 and int(flag.item()) == 0 and bool((ints[:, 1:] == 12345).all())
	assert bool((wsbuf[:off] == 0xff).all()) and bool((wsbuf[off + need:] == 0xff).all())
	# guards: behind each output and in the row pitch pads
	assert bool((sbuf[g:] == SENT).all())
	for view, buf, pitch, nr in ((U, ubuf, g + 3, rows), (V, vbuf, g + 7, cols)):
		flat = buf.clone()
		torch.as_strided(flat, (nr, g), (pitch, 1)).fill_(SENT)
		assert bool((flat == SENT).all()), "an element outside the [n x g] output was written"
	S, order = torch.sort(sigma, descending=True, stable=True)
	assert np.array_equal(S.cpu().numpy(), np.sort(float(root) * D)[::-1])
	svd = ops.SVD(U.index_select(1, order), S, V.index_select(1, order), sweeps, converged)
	# the same through the public call (its own scratch and outputs): equal bits
	pub = ops.svd_jacobi(Wd)
	assert pub.sweeps == 1 and pub.converged
	for a, b in ((pub.U, svd.U), (pub.S, svd.S), (pub.V, svd.V)):
		assert torch.equal(a.view(torch.int64), b.contiguous().view(torch.int64))
	X, rank = ops.pinv_from_svd(svd)
	assert rank == g and X.dtype == torch.float32 and tuple(X.shape) == (cols, rows)
	assert np.array_equal(X.cpu().numpy().view(np.uint32), X_want.astype(np.float32).view(np.uint32))
	# a cutoff between two singular values: d_j < 2^-3.5 goes
	Xt, rank_t = ops.pinv_from_svd(svd, rcond=2.0 ** -3.5)
	keep = D > 2.0 ** -3.5
	assert rank_t == int(keep.sum()) == 4 * (g // 7) + min(g % 7, 4)
	want_t = X_want.copy()
	if transposed:
		want_t[:, ~keep] = 0.0
	else:
		want_t[~keep, :] = 0.0
	assert np.array_equal(Xt.cpu().numpy().view(np.uint32), want_t.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
def test_exact_hadamard_block_bit_for_bit(ops, dtype, transposed):
	_exact_hadamard_block(ops, 64, 48, dtype, transposed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
def test_exact_hadamard_block_above_256_vectors(ops, dtype, transposed):
	"""g = 600: three passes of every loop over g (the copy of Vt, the maximum, the scaling and the rank count, the identity's grid), the third
	one ragged (600 = 2 * 256 + 88).  No rotation happens on this data, so the rotation of Vt is the generic cases' to test."""
	_exact_hadamard_block(ops, 1024, 600, dtype, transposed)


@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
def test_exact_hadamard_block_at_the_limit(ops, transposed):
	"""g = 2048 = ANNCUR_SVD_MAX_G with L = 4096: eight full passes over g, rows read twice (L above the register path), S = 64 d."""
	from anncur_amd import _lib
	assert _lib.SVD_MAX_G == 2048
	_exact_hadamard_block(ops, 4096, 2048, torch.float32, transposed)


# ------------------------------------------------------------------ 2. generic data
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generic_against_numpy_fp64(ops, shape):
	W, _, S_ref, _ = generic(*shape)
	svd = ops.svd_jacobi(torch.tensor(W).cuda())
	g = min(shape)
	assert svd.converged and svd.sweeps <= 30
	assert tuple(svd.U.shape) == (shape[0], g) and tuple(svd.V.shape) == (shape[1], g) and tuple(svd.S.shape) == (g,)
	S = svd.S.cpu().numpy()
	assert np.all(S[:-1] >= S[1:])
	r = ratios(W, S_ref, svd)
	print(f"svd {shape[0]} x {shape[1]}: sweeps {svd.sweeps}, error / (g 2^-53 sigma_max): " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
	for k, v in r.items():
		assert v <= C, (k, v)


def test_two_columns_of_equal_norm_take_the_45_degree_rotation(ops):
	"""[[2, 1], [1, 2]]: alpha == beta, so zeta == 0 and the rotation is t = 1 (the branch no random matrix takes); singular values 3 and 1."""
	W = np.array([[2.0, 1.0], [1.0, 2.0]], dtype=np.float32)
	svd = ops.svd_jacobi(torch.tensor(W).cuda())
	assert svd.converged and svd.sweeps == 2                             # one rotation, then a sweep that finds nothing to do
	r = ratios(W, np.array([3.0, 1.0]), svd)
	print("svd [[2, 1], [1, 2]]: error / (g 2^-53 sigma_max): " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
	for k, v in r.items():
		assert v <= C, (k, v)


LONG_SHAPES = [(5, 2048), (3, 2049), (2049, 3), (2, 8192), (300, 2100)]


@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_rows_on_both_sides_of_the_register_path(ops, shape):
	"""L = 2048 is the longest row a thread keeps in registers between the dot pass and the update, 2049 the first that is read twice, 8192
	the limit.  Few vectors, so a sweep is a handful of launches -- but for 300 x 2100: rows read twice TOGETHER with g > 256 (there the scale
	below is 1).  With g this small the term that counts is not g but sqrt(L): the rotation
	rule leaves |u_i . u_j| up to sqrt(L) 2^-53 by construction, and a sum of L products carries rounding of that order, so the figures are
	held to C max(g, sqrt(L)) 2^-53 sigma_max: the constant of the generic test on the larger of the two scales."""
	W, _, S_ref, _ = generic(*shape)
	svd = ops.svd_jacobi(torch.tensor(W).cuda())
	assert svd.converged
	g, L = min(shape), max(shape)
	scale = max(g, L ** 0.5) / g
	r = ratios(W, S_ref, svd)
	print(f"svd {shape[0]} x {shape[1]}: sweeps {svd.sweeps}, error / (g 2^-53 sigma_max): " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; allowed {C * scale:.0f}")
	for k, v in r.items():
		assert v <= C * scale, (k, v)
	again = ops.svd_jacobi(torch.tensor(W).cuda())
	assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in ((svd.U, again.U), (svd.S, again.S), (svd.V, again.V)))


# ------------------------------------------------------------------ 3. / 4. truncation against numpy
def _pinv_bound(X_ref, S_ref, rank, g):
	xm = np.abs(X_ref).max()
	return C * g * EPS * (S_ref[0] / S_ref[rank - 1]) * xm + 2.0 ** -24 * xm


def _truncation_between_two_singular_values(rows, g, rcond, seed):
	from anncur_amd import pinv
	rng = np.random.default_rng(seed)
	U0, _ = np.linalg.qr(rng.standard_normal((rows, g)))
	V0, _ = np.linalg.qr(rng.standard_normal((g, g)))
	W = ((U0 * np.logspace(0, -6, g)) @ V0.T).astype(np.float32)
	W64 = W.astype(np.float64)
	S_ref = np.linalg.svd(W64, compute_uv=False)
	rank_ref = int((S_ref > rcond * S_ref[0]).sum())
	assert 0 < rank_ref < g and np.abs(S_ref / (rcond * S_ref[0]) - 1.0).min() > 1e-3     # (the cutoff is not on a singular value)
	X_ref = np.linalg.pinv(W64, rcond=rcond)
	X, info = pinv.pinv_svd(torch.from_numpy(W).cuda(), rcond=rcond, return_info=True)
	assert info["converged"] and info["rank"] == rank_ref
	err, bound = np.abs(X.cpu().numpy().astype(np.float64) - X_ref).max(), _pinv_bound(X_ref, S_ref, rank_ref, g)
	print(f"truncated pinv {rows} x {g}: rank {info['rank']}, sweeps {info['sweeps']}, max|X - X_ref| = {err:.3e}, bound {bound:.3e}")
	assert err <= bound
	assert np.abs(info["singular_values"].cpu().numpy() - S_ref).max() <= C * g * EPS * S_ref[0]
	return info["rank"]


def test_truncation_between_two_singular_values(ops):
	_truncation_between_two_singular_values(96, 64, 10.0 ** -3.05, 7)


@pytest.mark.parametrize("rank", [152, 271])
def test_truncation_between_two_of_300_singular_values(ops, rank):
	"""g = 300: svd_scale_cols_kernel scales and counts over two passes.  The values are sorted descending, so with rank 152 the second pass
	(256 .. 299) must zero everything and count nothing, with rank 271 both passes keep and count.  The cutoff is the geometric mean of two
	neighbours of logspace(0, -6, 300); the fp32 rounding of W moves no singular value to within 2 % of it."""
	assert _truncation_between_two_singular_values(400, 300, 10.0 ** (-6.0 * (rank - 0.5) / 299.0), 8) == rank


def test_rank_deficient_block(ops):
	from anncur_amd import pinv
	W = np.random.default_rng(11).standard_normal((40, 12)).astype(np.float32)
	W[:, 7] = W[:, 3]        # two equal columns
	W[:, 5] = 0.0            # and a zero column
	W64 = W.astype(np.float64)
	S_ref = np.linalg.svd(W64, compute_uv=False)
	rank_ref = int((S_ref > 1e-10 * S_ref[0]).sum())
	assert rank_ref == 10
	X_ref = np.linalg.pinv(W64, rcond=1e-10)
	X, info = pinv.pinv_svd(torch.from_numpy(W).cuda(), rcond=1e-10, return_info=True)
	Xh = X.cpu().numpy().astype(np.float64)
	assert np.isfinite(Xh).all() and bool(torch.isfinite(info["singular_values"]).all())
	assert info["rank"] == rank_ref
	err, bound = np.abs(Xh - X_ref).max(), _pinv_bound(X_ref, S_ref, rank_ref, 12)
	print(f"rank-deficient 40 x 12: rank {info['rank']}, sweeps {info['sweeps']}, converged {info['converged']}, max|X - X_ref| = {err:.3e}, bound {bound:.3e}")
	assert err <= bound


# ------------------------------------------------------------------ 5. repeatability, the sweep cap, the fallback
def test_same_bits_on_every_call(ops):
	W = torch.tensor(generic(96, 192)[0]).cuda()
	a, b = ops.svd_jacobi(W), ops.svd_jacobi(W)
	assert a.sweeps == b.sweeps and a.converged and b.converged
	for x, y in ((a.U, b.U), (a.S, b.S), (a.V, b.V)):
		assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_sweep_cap_returns_unconverged_and_cur_falls_back_to_the_host(ops, monkeypatch, caplog):
	from anncur_amd import cur
	W = torch.tensor(generic(64, 64)[0]).cuda()
	svd = ops.svd_jacobi(W, max_sweeps=1)
	assert svd.sweeps == 1 and svd.converged is False
	real = ops.svd_jacobi
	monkeypatch.setattr(ops, "svd_jacobi", lambda M, max_sweeps=30: real(M, max_sweeps=1))
	with caplog.at_level(logging.INFO, logger="anncur_amd.cur"):
		info = {}
		X = cur._pinv(W, W.device, "svd", None, info)
	assert any("pinv svd" in r.getMessage() and "not converged" in r.getMessage() for r in caplog.records)
	assert info == {"singular_values": None, "rank": None}
	assert torch.equal(X.cpu(), cur._pinv_host(W))
