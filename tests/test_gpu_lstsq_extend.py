"""ops.LstsqState (anncur_lstsq_extend): the per-query Cholesky factor extended round by round.

The contract is bit equality with ops.lstsq_rows on the same rows after EVERY step, status included, so W and status are compared as uint32
views (NaN rows compare too).  Layout of every case: Rt is a view into a NaN-filled buffer (the pitch pad and the rows no id names are
NaN), ids and C are column slices of wider tensors (a row pitch above n), and W, status and the state buffer are filled with 0xff before
the first call -- the state is never pre-filled by the caller.
(1) Gaussian data against lstsq_rows, on sequences of sizes that restart inside a 16-block, cross a 64-row Gram tile, append one item, end
    at cap and run at a state pitch above the solve's own;  (2) signed Sylvester-Hadamard columns against the rational result, which needs
    no lstsq_rows;  (3) a duplicate id fails its query alone, for good;  (4) an item that raises max G_ii fails pivots accepted earlier;
(5) the timed variant.  Needs an MI355X."""
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


def nan_backed(Rt, named, pad=5):
	"""Rt [m x kq] on the device as a view into a NaN buffer of pitch kq + pad; the rows outside `named` are NaN too."""
	m, kq = Rt.shape
	buf = torch.full((m, kq + pad), float("nan"), dtype=torch.float32)
	rows = np.unique(np.asarray(named).reshape(-1))
	rows = rows[(rows >= 0) & (rows < m)]
	buf[rows, :kq] = torch.from_numpy(np.ascontiguousarray(Rt[rows], dtype=np.float32))
	return buf.cuda()[:, :kq]


def poisoned_out(Q, kq):
	W = torch.empty((Q, kq), dtype=torch.float32, device="cuda")
	status = torch.empty((Q,), dtype=torch.int32, device="cuda")
	W.view(torch.uint8).fill_(0xff)
	status.view(torch.uint8).fill_(0xff)
	return W, status


def new_state(ops, Rt, Q, cap, ridge):
	st = ops.LstsqState(Rt, Q, cap, ridge)
	st._state().fill_(0xff)
	return st


def step(st, ids, C, n, timings=None):
	"""One extend to n positions with poisoned outputs -> (W, status) as uint32 / int32 numpy arrays."""
	W, status = poisoned_out(st.Q, st.kq)
	st.extend(ids[:, :n], C[:, :n], out=(W, status), timings=timings)
	torch.cuda.synchronize()
	assert st.n == n
	return W.cpu().numpy().view(np.uint32), status.cpu().numpy()


def rows_ref(ops, Rt, ids, C, n, ridge):
	W, status = poisoned_out(ids.shape[0], Rt.shape[1])
	ops.lstsq_rows(Rt, ids[:, :n], C[:, :n], ridge, out=(W, status))
	torch.cuda.synchronize()
	return W.cpu().numpy().view(np.uint32), status.cpu().numpy()


# ---------------------------------------------------------------- (1) Gaussian data, bit-equal to lstsq_rows after every step
SEQUENCES = [(64, 32, (16, 32), 5),            # whole panels, cap = the final n
			 (100, 48, (13, 29, 30), 5),       # the partial block re-formed, a one-item step, state pitch 48 above the solve's 32
			 (100, 80, (64, 65, 80), 5),       # across a 64-row Gram tile
			 (500, 144, (100, 130), 5),
			 (320, 304, (256, 272, 300), 5),
			 (1536, 512, (448, 512), 2)]


def gaussian_rows(kq, steps, Q, seed):
	"""ids = a random permutation per query with holes at the first, a middle and the last position of the first segment (query 0) and one
	inside an appended segment (the last query)."""
	rng = np.random.default_rng(seed)
	n1, n = steps[0], steps[-1]
	m = 2 * n + 11
	Rt = rng.standard_normal((m, kq)).astype(np.float32)
	ids = np.stack([rng.permutation(m)[:n] for _ in range(Q)]).astype(np.int32)
	ids[0, [0, n1 // 2, n1 - 1]] = -1
	ids[Q - 1, n1 + (steps[1] - n1) // 2] = m + 3 if Q > 2 else -1     # (an id >= m is a hole too)
	C = rng.standard_normal((Q, n)).astype(np.float32)
	return Rt, ids, C


@pytest.mark.parametrize("ridge", [0.0, 0.5])
@pytest.mark.parametrize("kq,cap,steps,Q", SEQUENCES)
def test_gaussian_bit_equal_to_lstsq_rows_after_every_step(ops, kq, cap, steps, Q, ridge):
	for attempt in range(10):
		Rt_h, ids_h, C_h = gaussian_rows(kq, steps, Q, seed=1000 * (kq + cap) + attempt)
		Rt, ids, C = nan_backed(Rt_h, ids_h), torch.from_numpy(ids_h).cuda(), torch.from_numpy(C_h).cuda()
		refs = [rows_ref(ops, Rt, ids, C, n, ridge) for n in steps]
		if not any(status.any() for _, status in refs):     # a condition on lstsq_rows alone: a draw that fails it is replaced
			break
	else:
		raise AssertionError("no draw that lstsq_rows solves in 10 attempts")
	st = new_state(ops, Rt, Q, cap, ridge)
	assert st.cap == cap and st.n == 0
	for n, (W_ref, status_ref) in zip(steps, refs):
		W, status = step(st, ids, C, n)
		assert np.array_equal(status, status_ref) and not status.any(), (n, status)
		assert np.array_equal(W, W_ref), (n, int((W != W_ref).sum()))


# ---------------------------------------------------------------- (2) exact data, independent of lstsq_rows
def hadamard(g):
	H = np.array([[1]], dtype=np.int64)
	while H.shape[0] < g:
		H = np.block([[H, H], [H, -H]])
	assert H.shape[0] == g
	return H


def hadamard_rows(g, n, Q, seed, hole_pos):
	"""Q rows of n positions: the non-hole positions of row q hold, in random order, distinct item ids whose Rt rows are distinct columns of H_g
	under random signs.  -> (Rt host [m x g], ids int32 [Q x n], C fp32 [Q x n], contrib int64 [Q x n x g] = c_j col_j, zero at holes)."""
	rng = np.random.default_rng(seed)
	H = hadamard(g)
	real_pos = [j for j in range(n) if j not in set(hole_pos)]
	n_real = len(real_pos)
	assert n_real <= g
	m = 3 * n_real + 7
	cols = rng.permutation(g)[:n_real]
	item_of, sign = rng.permutation(m)[:n_real], rng.choice([-1, 1], n_real)
	Rt = np.zeros((m, g), dtype=np.float32)
	for t in range(n_real):
		Rt[item_of[t]] = sign[t] * H[:, cols[t]]
	ids = np.full((Q, n), -1, dtype=np.int32)
	C = rng.integers(-64, 65, (Q, n)).astype(np.float32)          # (values at holes: ignored)
	contrib = np.zeros((Q, n, g), dtype=np.int64)
	for q in range(Q):
		for j, t in zip(real_pos, rng.permutation(n_real)):
			ids[q, j] = item_of[t]
			contrib[q, j] = int(C[q, j]) * sign[t] * H[:, cols[t]]
	return Rt, ids, C, contrib


def exact_f32(S, d):
	w = S.astype(np.float64) / d
	assert np.array_equal(w.astype(np.float32).astype(np.float64), w)   # the rational result IS an fp32 number
	return w.astype(np.float32)


@pytest.mark.parametrize("ridge_mult", [0, 3])
def test_hadamard_bit_exact_at_every_step(ops, ridge_mult):
	# G = g I on the non-holes (+ 3 g I: 4 g I), every intermediate exact in fp64: W = (sum_{j < n} c_j col_j) / d at every step
	g, Q, steps = 64, 5, (16, 40, 64)
	Rt_h, ids_h, C_h, contrib = hadamard_rows(g, g, Q, seed=64 + ridge_mult, hole_pos=(0, 20, 63))     # one hole per segment
	Rt, ids, C = nan_backed(Rt_h, ids_h), torch.from_numpy(ids_h).cuda(), torch.from_numpy(C_h).cuda()
	st = new_state(ops, Rt, Q, g, float(ridge_mult * g))
	for n in steps:
		W, status = step(st, ids, C, n)
		assert not status.any()
		assert np.array_equal(W, exact_f32(contrib[:, :n].sum(axis=1), (1 + ridge_mult) * g).view(np.uint32)), n


# ---------------------------------------------------------------- (3) failure is per query and sticky
def test_duplicate_in_second_segment_fails_that_query_for_good(ops):
	g, Q, steps = 64, 5, (16, 40, 64)
	Rt_h, ids_h, C_h, contrib = hadamard_rows(g, g, Q, seed=3, hole_pos=(5, 30, 50))
	ids_h[2, 22] = ids_h[2, 1]                                     # two equal columns: the second pivot is exactly 0
	Rt, ids, C = nan_backed(Rt_h, ids_h), torch.from_numpy(ids_h).cuda(), torch.from_numpy(C_h).cuda()
	st = new_state(ops, Rt, Q, g, 0.0)
	keep, failed = [0, 1, 3, 4], np.array([0, 0, 1, 0, 0], dtype=np.int32)
	W, status = step(st, ids, C, 16)
	assert not status.any() and np.array_equal(W, exact_f32(contrib[:, :16].sum(axis=1), g).view(np.uint32))
	per_query = st._state().view(Q, -1)
	for n in steps[1:]:
		before = per_query[2].clone() if n == steps[2] else None
		W, status = step(st, ids, C, n)
		W_ref, status_ref = rows_ref(ops, Rt, ids, C, n, 0.0)
		assert np.array_equal(status, failed) and np.array_equal(status_ref, failed), (n, status, status_ref)
		assert np.isnan(W[2].view(np.float32)).all()
		assert np.array_equal(W, W_ref)                            # (the NaN row too: one bit pattern)
		assert np.array_equal(W[keep], exact_f32(contrib[keep, :n].sum(axis=1), g).view(np.uint32))
		if before is not None:
			assert torch.equal(per_query[2], before)               # a failed query's state is left as it is


# ---------------------------------------------------------------- (4) a grown maximum fails an old pivot
def test_grown_maximum_fails_an_old_pivot(ops):
	# items 0..15 = unit columns e_0..e_15 (pivots 1); item 16 = 2^21 e_16: G_ii = 2^42, threshold 2^-40 2^42 = 4 > 1; item 17 = e_16
	kq = 24
	Rt_h = np.zeros((20, kq), dtype=np.float32)
	Rt_h[np.arange(16), np.arange(16)] = 1.0
	Rt_h[16, 16], Rt_h[17, 16] = 2.0 ** 21, 1.0
	ids_h = np.stack([np.arange(17), np.r_[np.arange(16), 17]]).astype(np.int32)
	C_h = np.arange(1, 35, dtype=np.float32).reshape(2, 17)
	Rt, ids, C = nan_backed(Rt_h, ids_h), torch.from_numpy(ids_h).cuda(), torch.from_numpy(C_h).cuda()
	st = new_state(ops, Rt, 2, 17, 0.0)
	W, status = step(st, ids, C, 16)
	assert not status.any() and np.array_equal(W.view(np.float32)[:, :16], C_h[:, :16]) and not W[:, 16:].any()
	W, status = step(st, ids, C, 17)
	W_ref, status_ref = rows_ref(ops, Rt, ids, C, 17, 0.0)
	assert np.array_equal(status_ref, [1, 0]) and np.array_equal(status, status_ref) and np.array_equal(W, W_ref)
	assert np.isnan(W[0].view(np.float32)).all() and np.array_equal(W[1].view(np.float32)[:17], C_h[1])


# ---------------------------------------------------------------- (5) the timed variant
def test_timed_variant_returns_three_times_and_the_same_W(ops):
	kq, cap, steps, Q = 100, 48, (13, 29, 30), 5
	Rt_h, ids_h, C_h = gaussian_rows(kq, steps, Q, seed=77)
	Rt, ids, C = nan_backed(Rt_h, ids_h), torch.from_numpy(ids_h).cuda(), torch.from_numpy(C_h).cuda()
	plain, timed, times = new_state(ops, Rt, Q, cap, 0.5), new_state(ops, Rt, Q, cap, 0.5), []
	for n in steps:
		W, status = step(plain, ids, C, n)
		Wt, status_t = step(timed, ids, C, n, timings=times)
		assert np.array_equal(W, Wt) and np.array_equal(status, status_t)
	assert len(times) == len(steps)
	for ms in times:
		assert len(ms) == 3 and all(np.isfinite(t) and t >= 0.0 for t in ms)
