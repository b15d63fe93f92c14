"""ops.LstsqState.seed_shared (anncur_lstsq_seed_shared): a state seeded from the prefix that every query's rows share -- factored
once, copied to every slot -- and then extended.

The contract is bit equality after EVERY step with ops.lstsq_rows on the same rows and with an unseeded LstsqState, status included, so W and
status are compared as uint32 views (NaN rows compare too).  Layout as in tests/test_gpu_lstsq_extend.py: Rt is a view into a NaN-filled
buffer, ids and C are column slices of wider tensors, and W, status and the state buffer are filled with 0xff before the first call.
(1) Gaussian data on prefixes that end on a 16-block, inside one (p0 = 0: only the header of the seed survives; r0 = 16), on a Gram tile
    edge, with one query only and at the adaptive search's size;  (2) signed Sylvester-Hadamard columns against the rational result, which
    needs no lstsq_rows;  (3) a duplicate inside the shared list fails every query for good;  (4) failures of one query: a duplicate of an
    anchor, and an appended item that raises max G_ii above a shared pivot;  (5) the seed writes the prefix' rows and four header words and
    nothing else.  Needs an MI355X."""
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


def seeded_state(ops, Rt, Q, cap, ridge, shared):
	"""A 0xff-poisoned state seeded with `shared`, given in turn as a host list, a numpy array and an int32 tensor on the device."""
	st = new_state(ops, Rt, Q, cap, ridge)
	shared = np.asarray(shared)
	form = (len(shared) + Q) % 3
	assert st.seed_shared(shared.tolist() if form == 0 else shared.astype(np.int64) if form == 1 else torch.from_numpy(shared.astype(np.int32)).cuda()) is None
	assert st.n == len(shared)
	return st


def step(st, ids, C, n):
	"""One extend to n positions with poisoned outputs -> (W, status) as uint32 / int32 numpy arrays."""
	W, status = poisoned_out(st.Q, st.kq)
	st.extend(ids[:, :n], C[:, :n], out=(W, status))
	torch.cuda.synchronize()
	assert st.n == n
	return W.cpu().numpy().view(np.uint32), status.cpu().numpy()


def rows_ref(ops, Rt, ids, C, n, ridge):
	W, status = poisoned_out(ids.shape[0], Rt.shape[1])
	ops.lstsq_rows(Rt, ids[:, :n], C[:, :n], ridge, out=(W, status))
	torch.cuda.synchronize()
	return W.cpu().numpy().view(np.uint32), status.cpu().numpy()


def device_rows(Rt_h, ids_h, C_h, extra=3):
	"""-> (Rt NaN-backed, ids, C) on the device, ids and C as column slices of tensors `extra` columns wider (a row pitch above n)."""
	Q, n = ids_h.shape
	ids = torch.full((Q, n + extra), -7, dtype=torch.int32)
	C = torch.full((Q, n + extra), float("nan"), dtype=torch.float32)
	ids[:, :n], C[:, :n] = torch.from_numpy(ids_h), torch.from_numpy(C_h)
	return nan_backed(Rt_h, ids_h), ids.cuda()[:, :n], C.cuda()[:, :n]


# ---------------------------------------------------------------- (1) Gaussian data, bit-equal to lstsq_rows and to an unseeded state after every step
SEQUENCES = [(64, 40, 16, (24, 40), 5),           # aligned prefix
			 (100, 48, 13, (29, 30), 5),          # p0 = 0: nothing of the seed survives except the header; a one-item step
			 (100, 48, 24, (40,), 5),             # partial block re-formed, r0 = 16
			 (100, 80, 64, (65, 80), 5),          # prefix ends on a Gram tile edge
			 (100, 80, 70, (80,), 1),             # slot 0 is the only query
			 (500, 356, 256, (306, 356), 3)]      # the adaptive search's per-query shape (256 anchors, 50 a round, 500 anchor queries)


def gaussian_shared_rows(kq, n_sh, steps, Q, seed):
	"""ids = one shared prefix of n_sh distinct items without holes, then a random permutation of the other items per query, with a hole (-1)
	inside the first appended segment of query 0 and, for Q > 1, an id >= m inside the last appended segment of the last query."""
	rng = np.random.default_rng(seed)
	n = steps[-1]
	m = 2 * n + 11
	Rt = rng.standard_normal((m, kq)).astype(np.float32)
	perm = rng.permutation(m)
	shared, rest = perm[:n_sh], perm[n_sh:]
	ids = np.stack([np.r_[shared, rng.permutation(rest)[:n - n_sh]] for _ in range(Q)]).astype(np.int32)
	ids[0, n_sh + (steps[0] - n_sh) // 2] = -1
	if Q > 1:
		last0 = steps[-2] if len(steps) > 1 else n_sh
		ids[Q - 1, last0 + (n - last0) // 2] = m + 3                   # (an id >= m is a hole too)
	C = rng.standard_normal((Q, n)).astype(np.float32)
	return Rt, ids, C, shared.astype(np.int32)


@pytest.mark.parametrize("ridge", [0.0, 0.5])
@pytest.mark.parametrize("kq,cap,n_sh,steps,Q", SEQUENCES)
def test_gaussian_bit_equal_to_lstsq_rows_and_to_an_unseeded_state(ops, kq, cap, n_sh, steps, Q, ridge):
	for attempt in range(10):
		Rt_h, ids_h, C_h, shared = gaussian_shared_rows(kq, n_sh, steps, Q, seed=1000 * (kq + cap + n_sh) + attempt)
		Rt, ids, C = device_rows(Rt_h, ids_h, C_h)
		refs = [rows_ref(ops, Rt, ids, C, n, ridge) for n in steps]
		if not any(status.any() for _, status in refs):     # a condition on lstsq_rows alone: a draw that fails it is replaced
			break
	else:
		raise AssertionError("no draw that lstsq_rows solves in 10 attempts")
	assert (ids_h[:, :n_sh] == shared[None, :]).all() and shared.min() >= 0      # the prefix has no hole
	st, plain = seeded_state(ops, Rt, Q, cap, ridge, shared), new_state(ops, Rt, Q, cap, ridge)
	assert st.cap == cap and st.n == n_sh and plain.n == 0
	for n, (W_ref, status_ref) in zip(steps, refs):
		W, status = step(st, ids, C, n)
		W_plain, status_plain = step(plain, ids, C, n)
		assert np.array_equal(status, status_ref) and np.array_equal(status_plain, status_ref) and not status.any(), (n, status, status_plain)
		assert np.array_equal(W, W_ref), (n, int((W != W_ref).sum()))
		assert np.array_equal(W, W_plain), (n, int((W != W_plain).sum()))


# ---------------------------------------------------------------- (2) exact data, independent of lstsq_rows
def hadamard(g):
	H = np.array([[1]], dtype=np.int64)
	while H.shape[0] < g:
		H = np.block([[H, H], [H, -H]])
	assert H.shape[0] == g
	return H


def hadamard_shared_rows(g, n, n_sh, Q, seed, hole_pos):
	"""Q rows of n positions over distinct item ids whose Rt rows are distinct columns of H_g under random signs: the first n_sh positions hold
	the same items in every row (no holes), the other non-hole positions the remaining items in a random order per row.
	-> (Rt host [m x g], ids int32 [Q x n], C fp32 [Q x n], contrib int64 [Q x n x g] = c_j col_j, zero at holes)."""
	rng = np.random.default_rng(seed)
	H = hadamard(g)
	assert all(j >= n_sh for j in hole_pos)
	real_pos = [j for j in range(n_sh, n) if j not in set(hole_pos)]
	n_real = n_sh + len(real_pos)
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
		order = np.r_[np.arange(n_sh), n_sh + rng.permutation(n_real - n_sh)]
		for j, t in zip(list(range(n_sh)) + real_pos, order):
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
	g, n_sh, Q, steps = 64, 16, 5, (40, 64)
	Rt_h, ids_h, C_h, contrib = hadamard_shared_rows(g, g, n_sh, Q, seed=64 + ridge_mult, hole_pos=(20, 63))     # one hole per appended segment
	assert (ids_h[:, :n_sh] == ids_h[0, :n_sh]).all() and ids_h[:, :n_sh].min() >= 0
	Rt, ids, C = device_rows(Rt_h, ids_h, C_h)
	st = seeded_state(ops, Rt, Q, g, float(ridge_mult * g), ids_h[0, :n_sh])
	for n in steps:
		W, status = step(st, ids, C, n)
		assert not status.any()
		assert np.array_equal(W, exact_f32(contrib[:, :n].sum(axis=1), (1 + ridge_mult) * g).view(np.uint32)), n


# ---------------------------------------------------------------- (3) a rank-deficient shared block fails every query, for good
def test_duplicate_inside_the_shared_list_fails_every_query_at_every_step(ops):
	g, n_sh, Q, steps = 64, 16, 5, (40, 64)
	Rt_h, ids_h, C_h, _ = hadamard_shared_rows(g, g, n_sh, Q, seed=5, hole_pos=(30, 50))
	ids_h[:, 9] = ids_h[:, 2]                                      # two equal columns in the shared block: the second pivot is exactly 0
	Rt, ids, C = device_rows(Rt_h, ids_h, C_h)
	st = seeded_state(ops, Rt, Q, g, 0.0, ids_h[0, :n_sh])        # (duplicates are not a host error)
	state = st._state()
	for n in steps:
		before = state.clone() if n == steps[1] else None
		W, status = step(st, ids, C, n)
		W_ref, status_ref = rows_ref(ops, Rt, ids, C, n, 0.0)
		assert status_ref.all() and np.array_equal(status, status_ref) and np.array_equal(status, np.ones(Q, dtype=np.int32)), (n, status, status_ref)
		assert np.isnan(W.view(np.float32)).all() and np.array_equal(W, W_ref)          # (the NaN rows: one bit pattern)
		if before is not None:
			assert torch.equal(state, before)                      # failed queries' states are left as they are


# ---------------------------------------------------------------- (4) failure of one query
def test_appended_duplicate_of_an_anchor_fails_that_query_alone_for_good(ops):
	g, n_sh, Q, steps = 64, 16, 5, (40, 64)
	Rt_h, ids_h, C_h, contrib = hadamard_shared_rows(g, g, n_sh, Q, seed=3, hole_pos=(30, 50))
	ids_h[2, 22] = ids_h[2, 1]                                     # query 2 appends a copy of anchor 1: its pivot is exactly 0
	Rt, ids, C = device_rows(Rt_h, ids_h, C_h)
	st = seeded_state(ops, Rt, Q, g, 0.0, ids_h[0, :n_sh])
	keep, failed = [0, 1, 3, 4], np.array([0, 0, 1, 0, 0], dtype=np.int32)
	per_query = st._state().view(Q, -1)
	for n in steps:
		before = per_query[2].clone() if n == steps[1] else None
		W, status = step(st, ids, C, n)
		W_ref, status_ref = rows_ref(ops, Rt, ids, C, n, 0.0)
		assert np.array_equal(status, failed) and np.array_equal(status_ref, failed), (n, status, status_ref)
		assert np.isnan(W[2].view(np.float32)).all()
		assert np.array_equal(W, W_ref)                            # (the NaN row too: one bit pattern)
		assert np.array_equal(W[keep], exact_f32(contrib[keep, :n].sum(axis=1), g).view(np.uint32))
		if before is not None:
			assert torch.equal(per_query[2], before)               # a failed query's state is left as it is


def test_grown_maximum_fails_a_shared_pivot_in_that_query_alone(ops):
	# the shared items 0..15 = unit columns e_0..e_15 (pivots 1, the master's smallest pivot); item 16 = 2^21 e_16: G_ii = 2^42, threshold
	# 2^-40 2^42 = 4 > 1 -- query 0 appends it and fails on a shared pivot; item 17 = e_16 -- query 1 appends it and succeeds
	kq = 24
	Rt_h = np.zeros((20, kq), dtype=np.float32)
	Rt_h[np.arange(16), np.arange(16)] = 1.0
	Rt_h[16, 16], Rt_h[17, 16] = 2.0 ** 21, 1.0
	ids_h = np.stack([np.arange(17), np.r_[np.arange(16), 17]]).astype(np.int32)
	C_h = np.arange(1, 35, dtype=np.float32).reshape(2, 17)
	Rt, ids, C = device_rows(Rt_h, ids_h, C_h)
	st = seeded_state(ops, Rt, 2, 17, 0.0, np.arange(16))
	W, status = step(st, ids, C, 17)
	W_ref, status_ref = rows_ref(ops, Rt, ids, C, 17, 0.0)
	assert np.array_equal(status_ref, [1, 0]) and np.array_equal(status, status_ref) and np.array_equal(W, W_ref)
	assert np.isnan(W[0].view(np.float32)).all() and np.array_equal(W[1].view(np.float32)[:17], C_h[1])


# ---------------------------------------------------------------- (5) what the seed writes
def test_seed_alone_writes_the_prefix_rows_and_the_header_only(ops):
	kq, cap, n_sh, Q = 100, 80, 24, 5
	Rt_h, ids_h, C_h, shared = gaussian_shared_rows(kq, n_sh, (40,), Q, seed=11)
	Rt, _, _ = device_rows(Rt_h, ids_h, C_h)
	st = seeded_state(ops, Rt, Q, cap, 0.0, shared)
	torch.cuda.synchronize()
	capp, gp = 80, 32
	raw = st._state().cpu().numpy().view(np.uint64).reshape(Q, (capp + 2) * capp + 16)
	poison = np.uint64(0xffffffffffffffff)
	rows, hdr = raw[:, :(capp + 2) * capp].reshape(Q, capp + 2, capp), raw[:, (capp + 2) * capp:]
	assert (rows[:, gp:] == poison).all()                          # the matrix rows at or beyond ceil16(n_sh), the row of z, the row of y
	assert (rows[:, :gp, gp:] == poison).all()                     # the columns beyond the prefix
	assert (hdr[:, 4:] == poison).all()
	# every slot holds slot 0's factor (the lower triangle) and its header: largest diagonal, smallest pivot, status 0, no valid entry of z
	low = np.tril(np.ones((gp, gp), dtype=bool))
	assert (rows[:, :gp, :gp][:, low] != poison).all()
	assert (rows[:, :gp, :gp][:, low] == rows[0, :gp, :gp][low][None, :]).all() and (hdr[:, :4] == hdr[0, :4][None, :]).all()
	d = hdr[0, :4].view(np.float64)
	G = Rt_h[shared].astype(np.float64) @ Rt_h[shared].astype(np.float64).T
	assert np.isclose(d[0], G.diagonal().max(), rtol=1e-12) and 0.0 < d[1] <= d[0] and d[2] == 0.0 and d[3] == 0.0
	L = rows[0, :gp, :gp].view(np.float64)[:n_sh, :n_sh]
	assert np.allclose(np.tril(L) @ np.tril(L).T, G, rtol=1e-10, atol=1e-10 * d[0])
