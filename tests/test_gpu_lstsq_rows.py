"""ops.lstsq_rows (anncur_lstsq_rows): the batched per-query least squares of the adaptive search.

(a) Bit for bit on exact data.  The gathered columns are signed columns of a Sylvester-Hadamard matrix, so every Gram matrix is a multiple
of the identity with a power of two as square root, every intermediate is exact in fp64 and W must equal the rational result
(sum_j c_j col_j) / d rounded to fp32 -- here exactly representable.  Layout of every case: Rt is a view into a NaN-filled buffer (pitch pad
and the rows no id names are NaN), ids in random order, holes in the first, middle and last position, workspace and W filled with 0xff,
Q in {1, 5}, the chunked path forced by a byte cap of three queries (chunks of 3 and 2).  Sizes: g = 16, 64, 256 throughout, and each closed
form once more at the call's limits -- g = 512 on the item side (kq = 1024) and on the query side (kq = 512, with and without holes, and with
a ridge at n = 2048), kq = 4096.
(b) Against fp64 numpy on Gaussian data, with the bound derived in the issue: normal equations in fp64 err by at most
cond(G) g 2^-53 <= 2^10 2^9 2^-53 = 2^-34 relative to ||w||_2 where cond_2(R_S) <= 32 (asserted here on the host, from the reference alone; a
draw that fails is replaced), plus one fp32 rounding:  |W - w| <= 2^-24 |w| + 2^-30 ||w||_2  elementwise (16x margin on the 2^-34).
Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=None)
def hadamard(g):
	"""(shared between the cases and never written to)"""
	H = np.array([[1]], dtype=np.int64)
	while H.shape[0] < g:
		H = np.block([[H, H], [H, -H]])
	assert H.shape[0] == g
	H.setflags(write=False)
	return H


def nan_backed_rt(rows_by_id, m, kq, pad=5):
	"""Rt [m x kq] as a view into a NaN buffer of pitch kq + pad; only the rows in rows_by_id (id -> fp32 vector) are finite."""
	buf = torch.full((m, kq + pad), float("nan"), dtype=torch.float32)
	for i, v in rows_by_id.items():
		buf[i, :kq] = torch.from_numpy(np.asarray(v, dtype=np.float32))
	return buf.cuda()[:, :kq]


def hadamard_case(kq, cols, Q, seed, hole_pos=()):
	"""Q rows of n = len(cols) + len(hole_pos) positions; the non-hole positions of row q hold, in random order, distinct item ids whose Rt
	rows are the columns `cols` of H_kq under random signs.  -> (Rt, ids int32 [Q x n], C fp32 [Q x n], S int64 [Q x kq] = sum_j c_j col_j)."""
	rng = np.random.default_rng(seed)
	H = hadamard(kq)
	n_real, n = len(cols), len(cols) + len(hole_pos)
	m = 3 * n_real + 7
	item_of = rng.permutation(m)[:n_real]                       # item id that carries cols[t]
	sign = rng.choice([-1, 1], n_real)
	rows = {int(item_of[t]): sign[t] * H[:, cols[t]] for t in range(n_real)}
	ids = np.full((Q, n), -1, dtype=np.int32)
	C = rng.integers(-64, 65, (Q, n)).astype(np.float32)          # (values at holes: ignored)
	S = np.zeros((Q, kq), dtype=np.int64)
	real_pos = [j for j in range(n) if j not in set(hole_pos)]
	for q in range(Q):
		order = rng.permutation(n_real)
		for j, t in zip(real_pos, order):
			ids[q, j] = item_of[t]
			S[q] += int(C[q, j]) * sign[t] * H[:, cols[t]]
	return nan_backed_rt(rows, m, kq), torch.from_numpy(ids).cuda(), torch.from_numpy(C).cuda(), S


def run_poisoned(ops, Rt, ids, C, ridge, chunked):
	"""lstsq_rows with W, status and the workspace filled with 0xff first; chunked: a byte cap of three queries."""
	Q, n = ids.shape
	kq = Rt.shape[1]
	per_query = ops.lstsq_workspace_bytes(1, n, kq)
	assert per_query > 0
	cap = 3 * per_query if chunked else ops.LSTSQ_WS_LIMIT_BYTES
	ops._Workspace.get(min(Q, 3 if chunked else Q) * per_query, Rt.device).fill_(0xff)
	W = torch.empty((Q, kq), dtype=torch.float32, device=Rt.device)
	status = torch.empty((Q,), dtype=torch.int32, device=Rt.device)
	W.view(torch.uint8).fill_(0xff)
	status.view(torch.uint8).fill_(0xff)
	ops.lstsq_rows(Rt, ids, C, ridge, max_bytes=cap, out=(W, status))
	torch.cuda.synchronize()
	return W.cpu().numpy(), status.cpu().numpy()


def holes3(n_real):
	"""Hole positions first, middle, last of a row with n_real real entries and three holes."""
	n = n_real + 3
	return (0, n // 2, n - 1)


def exact_f32(S, d):
	w = S.astype(np.float64) / d
	assert np.array_equal(w.astype(np.float32).astype(np.float64), w)   # the rational result IS an fp32 number
	return w.astype(np.float32)


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("g", [16, 64, 256])
def test_item_side_hadamard_bit_exact(ops, g, Q, chunked):
	# n = g positions: holes first / middle / last, the other g - 3 hold distinct signed columns of H_g; G = g I on them
	pos = (0, g // 2, g - 1)
	cols = list(np.random.default_rng(g).permutation(g)[:g - 3])
	Rt, ids, C, S = hadamard_case(g, cols, Q, seed=10 * g + Q, hole_pos=pos)
	assert ids.shape[1] == g
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, chunked)
	assert np.array_equal(status, np.zeros(Q, dtype=np.int32))
	assert np.array_equal(W.view(np.uint32), exact_f32(S, g).view(np.uint32))
	# no holes: all g columns
	Rt, ids, C, S = hadamard_case(g, list(range(g)), Q, seed=11 * g + Q)
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, chunked)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, g).view(np.uint32))


@pytest.mark.parametrize("Q", [1, 5])
def test_item_side_wide_hadamard_bit_exact(ops, Q):
	# n = 16 < kq = 64: 13 columns of H_64 and three holes; G = 64 I
	cols = list(np.random.default_rng(5).permutation(64)[:13])
	Rt, ids, C, S = hadamard_case(64, cols, Q, seed=64 + Q, hole_pos=(0, 8, 15))
	assert ids.shape[1] == 16
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 64).view(np.uint32))


@pytest.mark.parametrize("with_holes", [False, True])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("kq", [8, 32, 128])
def test_query_side_hadamard_bit_exact(ops, kq, Q, with_holes):
	# R_S = [H | H] under signs: G = 2 kq I = 4^j I, w = R_S c^T / (2 kq).  A hole must contribute NOTHING, so the three holes are extra
	# positions (n = 2 kq + 3) around the 2 kq real ones; without them n = 2 kq.
	cols = list(range(kq)) * 2
	Rt, ids, C, S = hadamard_case(kq, cols, Q, seed=7 * kq + Q, hole_pos=holes3(2 * kq) if with_holes else ())
	assert ids.shape[1] == 2 * kq + (3 if with_holes else 0) > kq
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 2 * kq).view(np.uint32))


@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("g", [16, 64, 256])
def test_item_side_ridge_hadamard_bit_exact(ops, g, Q):
	# lambda = 3 g: G + lambda I = 4 g I, square root 2 sqrt(g)
	pos = (0, g // 2, g - 1)
	cols = list(np.random.default_rng(g + 1).permutation(g)[:g - 3])
	Rt, ids, C, S = hadamard_case(g, cols, Q, seed=13 * g + Q, hole_pos=pos)
	W, status = run_poisoned(ops, Rt, ids, C, 3.0 * g, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 4 * g).view(np.uint32))


# The same closed forms at the limits of the call: g = ANNCUR_LSTSQ_MAX_G = 512 on either side (the ninth row block of the factorisation's
# MAXBLK), kq = ANNCUR_LSTSQ_MAX_KQ = 4096 and n = ANNCUR_MAX_TOPK = 2048.  Q = 5 runs chunked (3 + 2).
@pytest.mark.parametrize("Q", [1, 5])
def test_item_side_g512_hadamard_bit_exact(ops, Q):
	# n = 512 positions on kq = 1024: 509 signed columns of H_1024 and holes first / middle / last; G = 1024 I
	from anncur_amd import _lib
	assert _lib.LSTSQ_MAX_G == 512
	cols = list(np.random.default_rng(512).permutation(1024)[:509])
	Rt, ids, C, S = hadamard_case(1024, cols, Q, seed=5120 + Q, hole_pos=(0, 256, 511))
	assert ids.shape[1] == 512
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 1024).view(np.uint32))


@pytest.mark.parametrize("Q", [1, 5])
def test_item_side_kq4096_hadamard_bit_exact(ops, Q):
	# n = 64 positions on kq = 4096 = ANNCUR_LSTSQ_MAX_KQ: 61 signed columns of H_4096 and three holes; G = 4096 I
	from anncur_amd import _lib
	assert _lib.LSTSQ_MAX_KQ == 4096
	cols = list(np.random.default_rng(4096).permutation(4096)[:61])
	Rt, ids, C, S = hadamard_case(4096, cols, Q, seed=4096 + Q, hole_pos=(0, 32, 63))
	assert ids.shape[1] == 64
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 4096).view(np.uint32))


@pytest.mark.parametrize("with_holes", [False, True])
@pytest.mark.parametrize("Q", [1, 5])
def test_query_side_kq512_hadamard_bit_exact(ops, Q, with_holes):
	# R_S = [H_512 | H_512] under signs: g = kq = 512, G = 1024 I; the three holes are extra positions (n = 1027)
	cols = list(range(512)) * 2
	Rt, ids, C, S = hadamard_case(512, cols, Q, seed=7 * 512 + Q, hole_pos=holes3(1024) if with_holes else ())
	assert ids.shape[1] == 1024 + (3 if with_holes else 0)
	W, status = run_poisoned(ops, Rt, ids, C, 0.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 1024).view(np.uint32))


@pytest.mark.parametrize("Q", [1, 5])
def test_query_side_ridge_at_the_longest_list_bit_exact(ops, Q):
	# four copies of H_512: n = 2048 = ANNCUR_MAX_TOPK, G = 2048 I, lambda = 2048: G + lambda I = 4096 I
	from anncur_amd import _lib
	assert _lib.MAX_TOPK == 2048
	cols = list(range(512)) * 4
	Rt, ids, C, S = hadamard_case(512, cols, Q, seed=9 * 512 + Q)
	assert ids.shape[1] == 2048
	W, status = run_poisoned(ops, Rt, ids, C, 2048.0, Q == 5)
	assert not status.any() and np.array_equal(W.view(np.uint32), exact_f32(S, 4096).view(np.uint32))


@pytest.mark.parametrize("g", [16, 64, 256])
def test_planted_duplicate_fails_that_query_only(ops, g):
	# two equal rows of G make the second pivot exactly 0, whatever the threshold: status 1 and a NaN row, the neighbours bit-equal
	pos = (0, g // 2, g - 1)
	cols = list(np.random.default_rng(g + 2).permutation(g)[:g - 3])
	Rt, ids, C, S = hadamard_case(g, cols, 5, seed=17 * g, hole_pos=pos)
	ids_h = ids.cpu().numpy().copy()
	ids_h[2, g - 2] = ids_h[2, 1]
	for chunked in (False, True):
		W, status = run_poisoned(ops, Rt, torch.from_numpy(ids_h).cuda(), C, 0.0, chunked)
		assert np.array_equal(status, np.array([0, 0, 1, 0, 0], dtype=np.int32))
		assert np.isnan(W[2]).all()
		keep = [0, 1, 3, 4]
		assert np.array_equal(W[keep].view(np.uint32), exact_f32(S, g)[keep].view(np.uint32))


# ---------------------------------------------------------------- (b) Gaussian data against fp64 numpy
ITEM_SIDE = [(100, 1), (100, 15), (100, 17), (100, 33), (64, 16), (500, 130)]
QUERY_SIDE = [(16, 64), (15, 100), (33, 100), (100, 300)]


def reference_w(Rs, c, lam):
	"""w = argmin ||w Rs - c||^2 + lam ||w||^2 in fp64 by the SVD (lam = 0: c . pinv(Rs)); -> (w, cond_2(Rs))."""
	U, s, Vt = np.linalg.svd(Rs, full_matrices=False)          # Rs = U diag(s) Vt, kq x n_q
	f = s / (s * s + lam)
	return ((c @ Vt.T) * f) @ U.T, s[0] / s[-1]


def gaussian_case(kq, n, Q, seed, holes):
	"""A draw whose every used R_S has cond_2 <= 32 by the fp64 reference (checked for lam = 0, the harder case); a failing draw is replaced."""
	for attempt in range(20):
		rng = np.random.default_rng(1000 * seed + attempt)
		m = 2 * n + 11
		Rt = rng.standard_normal((m, kq)).astype(np.float32)
		ids = np.stack([rng.permutation(m)[:n] for _ in range(Q)]).astype(np.int32)
		if holes and n >= 4:
			ids[0, [0, n // 2, n - 1]] = -1
			if Q > 2: ids[2, rng.integers(0, n)] = -1
		C = rng.standard_normal((Q, n)).astype(np.float32)
		conds = [reference_w(Rt[r[r >= 0]].astype(np.float64).T, c[r >= 0].astype(np.float64), 0.0)[1] for r, c in zip(ids, C)]
		if max(conds) <= 32:
			return Rt, ids, C
	raise AssertionError("no well-conditioned draw in 20 attempts")


def check_gaussian(ops, kq, n, Q, lam, holes):
	Rt, ids, C = gaussian_case(kq, n, Q, seed=kq * 7 + n, holes=holes)
	buf = torch.full((Rt.shape[0], kq + 3), float("nan"), dtype=torch.float32)
	buf[:, :kq] = torch.from_numpy(Rt)
	W, status = run_poisoned(ops, buf.cuda()[:, :kq], torch.from_numpy(ids).cuda(), torch.from_numpy(C).cuda(), lam, False)
	assert not status.any()
	for q in range(Q):
		keep = ids[q] >= 0
		Rs, c = Rt[ids[q][keep]].astype(np.float64).T, C[q][keep].astype(np.float64)
		w, cond = reference_w(Rs, c, lam)
		assert cond <= 32
		err, bound = np.abs(W[q].astype(np.float64) - w), 2.0 ** -24 * np.abs(w) + 2.0 ** -30 * np.linalg.norm(w)
		print(f"kq={kq} n={n} lam={lam} q={q} cond={cond:.2f} max err/bound = {(err / bound).max():.3f}")
		assert (err <= bound).all(), (kq, n, lam, q, float((err / bound).max()))
		if n <= kq and lam == 0.0:   # interpolation: the fp32 rounding of W propagated
			Wq = W[q].astype(np.float64)
			res, rb = np.abs(Wq @ Rs - c), 2.0 ** -23 * (np.abs(Wq) @ np.abs(Rs)) + 2.0 ** -30 * np.linalg.norm(c)
			assert (res <= rb).all(), (kq, n, q, float((res / rb).max()))


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("kq,n", ITEM_SIDE + QUERY_SIDE)
def test_gaussian_against_numpy(ops, kq, n, lam):
	check_gaussian(ops, kq, n, Q=4, lam=lam, holes=True)
	check_gaussian(ops, kq, n, Q=3, lam=lam, holes=False)


def test_gaussian_g512(ops):
	check_gaussian(ops, 1536, 512, Q=3, lam=0.0, holes=True)
