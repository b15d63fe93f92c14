"""The speculative start of the wave-per-row exact scan (csrc/topk.hip, rowwise_topk_wave_kernel) against plain numpy
(tests/topk_numpy.py), bit for bit, and its restart counters against a host prediction, exactly.

The scan may start a row from the r-th largest of the 512 group maxima of the row's first 512 16-byte vectors -- a guess -- instead of the
k-th largest -- a bound --, checks the guess at the block boundary nearest a quarter of the row and at the row's end, and scans the row again
from the bound where the guess was too high.  Whatever the rank, the result is the one of tests/topk_numpy.py: score descending, then the
smaller index, NaN never, -inf an ordinary candidate, (-inf, -1) padding.

Conventions of tests/test_gpu_rowwise_topk_exact.py: every matrix is an interior view of a larger buffer whose every other element is POISON
(+inf, NaN, 3e38 in turn), so a read outside a row -- the restart's second pass over it included -- stays inside the test's allocation and wins
the top-k; data is built from integer bit patterns; nothing has a tolerance.

Shapes, for both dtypes, Q = 64 rows: I = 4 n_seed (the shortest row the library speculates on; n_seed = 4096 bf16 / 2048 fp32 elements),
4 n_seed + one block of the stream + 5, and 40 000; aligned rows and a layout whose rows' 16-byte grid starts 0 .. VEC - 1 elements into the
row in turn (so 1 and VEC - 1 among them); k = 1, 64, 65, 100, 128.  One reference (the 128 best of every row) per matrix serves all k.

The host prediction (_predict): the kernel's own seed -- the r-th largest group-maximum key with an all-NaN group keyed 0, the fp32 just below
it, the denormal rule --, then the count of the row's numbers strictly above that threshold: a speculative row restarts iff fewer than k / 8 of
them lie before the quarter mark (where the clamp-free loop reaches it), or fewer than k in the whole row.  (Neither test needs to know
whether a compaction ran: one runs only above the trigger, which is above k.)

Where the library's rank is 0 for a (shape, k) -- k = 1 everywhere, k = 64 and 65 at I = 4 n_seed, where the rank would exceed k / 2 -- the
launch runs the kernel without the restart loop and both counters stay zero; the tests assert that too.

k = 1 never speculates: a forced rank of 1 IS the valid seed there (rank k), so "every row restarts" in the forced-rank case reads "every
row restarts for k >= 2, none for k = 1"; the auto rank is 0 for k = 1 (r >= 2 > k / 2).

iid rows alone restart about once in a hundred thousand, so a set of 64 holds no restarting row for any seed one could search for: the iid case
plants the row's r + 3 best elements in distinct seed groups of every other row (the rest of the row stays a random permutation), and the
host prediction -- not the device -- shows that such a set holds both kinds.
Needs an MI355X."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
VEC = {F32: 4, BF16: 8}
Q = 64
KS = (1, 64, 65, 100, 128)
KMAX = 128
SEED_VECS = tn.SEED_VECS            # 512
STEP_VECS, BLOCK_STEPS = 64, 8      # vectors per step of the wave, steps per block of the stream


def _n_seed(dtype):
	return SEED_VECS * VEC[dtype]


def _lengths(dtype):
	n = _n_seed(dtype)
	return {"4seed": 4 * n, "4seed+block+5": 4 * n + STEP_VECS * BLOCK_STEPS * VEC[dtype] + 5, "40000": 40000}


CASES = [pytest.param(dt, name, mis, id=f"{'f32' if dt == F32 else 'bf16'}-{name}-{'misaligned' if mis else 'aligned'}")
		 for dt in (F32, BF16) for name in ("4seed", "4seed+block+5", "40000") for mis in (False, True)]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


@pytest.fixture(scope="module")
def auto_rank():
	from anncur_amd import _lib
	fn = _lib.load().anncur_internal_scan_spec_rank
	fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int]
	return lambda I, k, dtype: int(fn(I, k, _lib.F32 if dtype == F32 else _lib.BF16))


# ------------------------------------------------------------------ bits, the poisoned buffer
def _to_f32(bits, dtype):
	return tn.f32_from_bits(bits) if dtype == F32 else tn.bf16_bits_to_f32(bits)


def _to_bits(values, dtype):
	v = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
	return v.view(np.uint32).copy() if dtype == F32 else tn.f32_to_bf16_bits(v)


def _distinct_rows(rng, n_rows, I, dtype):
	"""Rows of I distinct values in random order: mixed-sign integers (fp32) / distinct finite bf16 patterns."""
	if dtype == F32:
		return [(rng.permutation(I) - I // 2).astype(np.float32).view(np.uint32).copy() for _ in range(n_rows)]
	return [tn.distinct_bf16_patterns(rng, I).copy() for _ in range(n_rows)]


def _poisoned_view(rows, I, dtype, misaligned, gpu):
	"""A = buffer[1 : 1 + R, c0 : c0 + I] on the GPU, poison everywhere else.  Aligned: base and pitch multiples of 16 bytes.  Misaligned:
	column offset 1 and a pitch that is odd in elements, so the head runs through 0 .. VEC - 1 down the rows."""
	v = VEC[dtype]
	if misaligned:
		c0, pitch = 1, I + v + 2
		pitch += 1 - pitch % 2
	else:
		c0, pitch = 2 * v, -(-(I + 4 * v) // v) * v
	R = len(rows)
	pat = np.array([0x7F800000, 0x7FC00000, 0x7F61B1E6], dtype=np.uint32)     # +inf, NaN, 3e38
	if dtype == BF16:
		pat = (pat >> 16).astype(np.uint16)
	buf = pat[np.arange((R + 2) * pitch) % 3].reshape(R + 2, pitch)
	for j, r in enumerate(rows):
		assert r.dtype == (np.uint32 if dtype == F32 else np.uint16) and r.size == I
		buf[1 + j, c0:c0 + I] = r
	t = torch.from_numpy(buf.view(np.int32 if dtype == F32 else np.int16)).to(gpu).view(dtype)
	assert t.data_ptr() % 16 == 0
	return t[1:1 + R, c0:c0 + I], t


def _heads(A):
	es = A.element_size()
	return [((16 - (A.data_ptr() + j * A.stride(0) * es) % 16) % 16) // es for j in range(A.shape[0])]


# ------------------------------------------------------------------ the host prediction
def _seed_tau(x, dtype, rank, head):
	"""The threshold the kernel's seed takes from the rank-th largest group maximum of the row's first 512 vectors (None: none -- the row is
	too short for a seed, or the maximum is -inf / an all-NaN group's key)."""
	vec = VEC[dtype]
	if (x.size - head) // vec < SEED_VECS:
		return None
	g = x[head:head + SEED_VECS * vec].reshape(SEED_VECS, vec)
	allnan = np.isnan(g).all(axis=1)
	gmax = np.fmax.reduce(np.where(allnan[:, None], np.float32(0), g), axis=1)          # fmax skips a NaN next to a number
	keys = np.where(allnan, np.uint32(0), tn.f32_sortable(gmax))
	if dtype == BF16:
		keys = keys & np.uint32(0xFFFF0000)                                              # the kernel's 16-bit key in the high half
	kth = int(np.sort(keys)[::-1][rank - 1])
	if kth <= 0x007FFFFF:                                                                # at or below the key of -inf: no threshold
		return None
	t = tn.f32_unsortable(kth - 1)
	if abs(t) < np.float32(1.17549435e-38):
		t = np.float32(-1.17549435e-38)
	return t


def _predict(x, dtype, k, rank, head):
	"""-> (row starts from a guess, row restarts) for one row given as float32 values."""
	if rank <= 0 or rank >= k:
		return False, False
	tau = _seed_tau(x, dtype, rank, head)
	if tau is None:
		return False, False
	vec = VEC[dtype]
	nvec = (x.size - head) // vec
	nsteps = -(-nvec // STEP_VECS)
	cp = max(((nsteps // 4 + BLOCK_STEPS // 2) // BLOCK_STEPS) * BLOCK_STEPS, BLOCK_STEPS)
	above = x > tau                                                                      # (NaN fails)
	if (cp + 2 * BLOCK_STEPS) * STEP_VECS <= nvec and int(above[:head + cp * STEP_VECS * vec].sum()) < k // 8:
		return True, True
	return True, int(above.sum()) < k


def _predict_rows(rows, dtype, k, rank, heads):
	p = [_predict(_to_f32(r, dtype), dtype, k, rank, h) for r, h in zip(rows, heads)]
	return sum(a for a, _ in p), sum(b for _, b in p)


# ------------------------------------------------------------------ running and checking
def _reference(rows, dtype):
	want_v = np.empty((len(rows), KMAX), dtype=np.float32)
	want_i = np.empty((len(rows), KMAX), dtype=np.int32)
	for j, r in enumerate(rows):
		want_v[j], want_i[j] = tn.topk_ref(_to_f32(r, dtype), KMAX)
	return want_v, want_i


def _assert_same(got, want_v, want_i, what):
	gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy()
	assert gv.dtype == np.float32 and gi.dtype == np.int32 and gv.shape == want_v.shape and gi.shape == want_i.shape
	bad = np.flatnonzero((gv.view(np.uint32) != want_v.view(np.uint32)).any(axis=1) | (gi != want_i).any(axis=1))
	if bad.size:
		j = int(bad[0])
		c = int(np.flatnonzero((gv[j].view(np.uint32) != want_v[j].view(np.uint32)) | (gi[j] != want_i[j]))[0])
		raise AssertionError(f"{what}: {bad.size} rows differ; row {j} place {c}: got ({gv[j, c]!r}, {gi[j, c]}) want ({want_v[j, c]!r}, {want_i[j, c]})")


def _run(ops, A, k, spec, gpu):
	stats = torch.zeros(2, dtype=torch.int32, device=gpu)
	got = ops.rowwise_topk(A, k, _spec=spec, _stats=stats)
	torch.cuda.synchronize()
	s = stats.cpu().numpy()
	return got, int(s[0]), int(s[1])


def _check(ops, gpu, rows, dtype, misaligned, ranks, what, want=None, ks=KS):
	"""Every k: the launch with ranks(k) (None = auto) and the launch with speculation off give the reference's rows, bit for bit and hence
	each other's; the counters equal the host prediction (off: both zero).  -> {k: (restarted, started)} as predicted."""
	I = rows[0].size
	A, _buf = _poisoned_view(rows, I, dtype, misaligned, gpu)
	heads = _heads(A)
	if misaligned:
		assert {1, VEC[dtype] - 1} <= set(heads)
	else:
		assert set(heads) == {0}
	want_v, want_i = want if want is not None else _reference(rows, dtype)
	out = {}
	for k in ks:
		forced, rank = ranks(k)
		started, restarted = _predict_rows(rows, dtype, k, rank, heads)
		got, s0, s1 = _run(ops, A, k, forced, gpu)
		_assert_same(got, want_v[:, :k], want_i[:, :k], f"{what} k={k} rank={rank}")
		assert (s0, s1) == (restarted, started), f"{what} k={k} rank={rank}: counters ({s0} restarted, {s1} started), predicted ({restarted}, {started})"
		off, z0, z1 = _run(ops, A, k, 0, gpu)
		_assert_same(off, want_v[:, :k], want_i[:, :k], f"{what} k={k} speculation off")
		assert (z0, z1) == (0, 0)
		assert torch.equal(off.values.view(torch.int32), got.values.view(torch.int32)) and torch.equal(off.indices, got.indices)
		out[k] = (restarted, started)
	return out


def _plant_best_in_seed(rng, row, dtype, m, head_max):
	"""Swap the row's m best elements into m distinct groups of the seed region (positions that lie in the region for every head)."""
	vec = VEC[dtype]
	x = _to_f32(row, dtype)
	best = np.argsort(-x.astype(np.float64), kind="stable")[:m]
	groups = rng.choice(np.arange(2, SEED_VECS - 2, 2), size=m, replace=False)   # (even: distinct groups of the grid whatever its head)
	for src, g in zip(best, groups):
		dst = head_max + g * vec + int(rng.integers(vec))
		if dst in best:
			continue
		row[src], row[dst] = row[dst], row[src]


# ------------------------------------------------------------------ 1: iid rows, auto rank
@pytest.mark.parametrize("dtype,length,misaligned", CASES)
def test_iid_rows_auto_rank_restarts_as_predicted(ops, gpu, auto_rank, dtype, length, misaligned):
	I = _lengths(dtype)[length]
	rng = np.random.default_rng([1, VEC[dtype], I, int(misaligned)])
	rows = _distinct_rows(rng, Q, I, dtype)
	rmax = max(auto_rank(I, k, dtype) for k in KS)
	assert rmax > 0
	for j in range(1, Q, 2):     # every other row: more of the row's best inside the seed region than any rank in use
		_plant_best_in_seed(rng, rows[j], dtype, rmax + 3, VEC[dtype])
	pred = _check(ops, gpu, rows, dtype, misaligned, lambda k: (None, auto_rank(I, k, dtype)), "iid")
	assert auto_rank(I, 1, dtype) == 0 and pred[1] == (0, 0)
	on = [k for k in KS if auto_rank(I, k, dtype) > 0]
	assert {100, 128} <= set(on)                                  # (k = 64, 65 are off at I = 4 n_seed: the rank would exceed k / 2)
	for k in KS[1:]:
		restarted, started = pred[k]
		if k in on:
			assert started == Q and 0 < restarted < Q, (k, pred[k])   # both kinds of row, by the host prediction alone
		else:
			assert pred[k] == (0, 0)


# ------------------------------------------------------------------ 2: forced rank 1, the maximum in the seed region; descending rows
@pytest.mark.parametrize("dtype,length,misaligned", CASES)
def test_forced_rank_one_restarts_every_row(ops, gpu, dtype, length, misaligned):
	I = _lengths(dtype)[length]
	rng = np.random.default_rng([2, VEC[dtype], I, int(misaligned)])
	rows = _distinct_rows(rng, Q, I, dtype)
	for j in range(Q // 2):
		_plant_best_in_seed(rng, rows[j], dtype, 1, VEC[dtype])
	for j in range(Q // 2, Q):   # descending: the maximum first, every later element below everything before it
		x = _to_f32(rows[j], dtype)
		rows[j] = rows[j][np.argsort(-x.astype(np.float64), kind="stable")]
	pred = _check(ops, gpu, rows, dtype, misaligned, lambda k: (1, 1), "forced rank 1")
	assert pred[1] == (0, 0)     # rank 1 at k = 1 is the valid seed
	for k in KS[1:]:
		assert pred[k] == (Q, Q), (k, pred[k])


# ------------------------------------------------------------------ 3: ascending rows
@pytest.mark.parametrize("dtype,length,misaligned", CASES)
def test_ascending_rows_never_restart(ops, gpu, auto_rank, dtype, length, misaligned):
	I = _lengths(dtype)[length]
	rng = np.random.default_rng([3, VEC[dtype], I, int(misaligned)])
	rows = _distinct_rows(rng, Q, I, dtype)
	for j in range(Q):
		x = _to_f32(rows[j], dtype)
		rows[j] = rows[j][np.argsort(x.astype(np.float64), kind="stable")]
	pred = _check(ops, gpu, rows, dtype, misaligned, lambda k: (None, auto_rank(I, k, dtype)), "ascending")
	for k in KS[1:]:
		assert pred[k] == ((0, Q) if auto_rank(I, k, dtype) > 0 else (0, 0)), (k, pred[k])
	assert pred[100] == (0, Q) and pred[128] == (0, Q)


# ------------------------------------------------------------------ 4: ties
@pytest.mark.parametrize("dtype,length,misaligned", CASES)
def test_ties(ops, gpu, auto_rank, dtype, length, misaligned):
	"""Rows 0..7 constant (one value per row, zero and negative ones among them).  Rows 8..35 two-valued: the larger value sits in exactly r
	seed groups (so it IS the r-th seed maximum) and in n_out places behind the region, r + n_out on both sides of k.  Rows 36..63: distinct
	values, k - 10 of them above a value that then occurs 3 k times, half of the copies inside the seed region, half behind it: the ten
	smallest indices among the copies win.  (r and k here are those of k = 100; the other k see the same rows.)"""
	I = _lengths(dtype)[length]
	vec, k0 = VEC[dtype], 100
	r0 = auto_rank(I, k0, dtype)
	assert 2 <= r0 <= k0 // 2
	rng = np.random.default_rng([4, vec, I, int(misaligned)])
	region = SEED_VECS * vec
	rows = []
	for j in range(8):
		rows.append(np.full(I, _to_bits([np.float32([3.0, -2.5, 0.0, 1.0, -0.5, 7.0, -1024.0, 0.25][j])], dtype)[0]))
	for j in range(28):
		lo, hi = _to_bits([np.float32(-1.5 if j % 2 else 2.0), np.float32(4.0)], dtype)
		row = np.full(I, lo)
		groups = rng.choice(np.arange(2, SEED_VECS - 2, 2), size=r0, replace=False)   # (even: distinct groups of the grid whatever its head)
		row[vec + groups * vec + rng.integers(vec, size=r0)] = hi
		n_out = (0, k0 - r0 - 1, k0 - r0, k0 - r0 + 1, 2 * k0, 5, 700)[j % 7]
		row[rng.choice(np.arange(region + vec, I), size=n_out, replace=False)] = hi
		rows.append(row)
	for row in _distinct_rows(rng, 28, I, dtype):
		x = _to_f32(row, dtype)
		order = np.argsort(-x.astype(np.float64), kind="stable")
		tie = row[order[k0 - 10]]
		row[rng.choice(np.arange(vec, region), size=3 * k0 // 2, replace=False)] = tie
		row[rng.choice(np.arange(region + vec, I), size=3 * k0 // 2, replace=False)] = tie
		rows.append(row)
	_check(ops, gpu, rows, dtype, misaligned, lambda k: (None, auto_rank(I, k, dtype)), "ties, auto rank")
	pred = _check(ops, gpu, rows, dtype, misaligned, lambda k: (r0, r0), "ties, rank of k = 100", ks=(k0,))
	assert 0 < pred[k0][0] < Q and pred[k0][1] == Q


# ------------------------------------------------------------------ 5: NaN vectors in the seed region, short rows, -inf rows
@pytest.mark.parametrize("dtype,length,misaligned", CASES)
def test_nan_vectors_in_the_seed_region(ops, gpu, auto_rank, dtype, length, misaligned):
	I = _lengths(dtype)[length]
	vec = VEC[dtype]
	rows = []
	for j in range(Q):
		m = (1, 12, 99, 100, 200, 250)[j % 6]
		rows.append(tn.nan_block_row(vec, I, 100 + j, m, tn.NAN_POS32 if j % 2 else tn.NAN_NEG32, misaligned))
	_check(ops, gpu, rows, dtype, misaligned, lambda k: (None, auto_rank(I, k, dtype)), "NaN vectors, auto rank")
	_check(ops, gpu, rows, dtype, misaligned, lambda k: (min(2, k), min(2, k)), "NaN vectors, rank 2")


@pytest.mark.parametrize("dtype,length,misaligned", CASES)
@pytest.mark.parametrize("k", KS[1:])
def test_rows_with_fewer_than_k_numbers_restart_and_pad(ops, gpu, dtype, length, misaligned, k):
	"""Even rows: NaN but for n < k numbers (-inf among them), at least two of them in distinct seed groups.  Odd rows: -inf but for k - 1
	finite numbers, the same: the k-th place goes to the first -inf.  Forced rank 2: every row starts from its second-largest seed maximum,
	finds fewer than k numbers above it, restarts, and the second pass pads / takes the -inf as the kernel always did."""
	I = _lengths(dtype)[length]
	vec = VEC[dtype]
	rng = np.random.default_rng([5, vec, I, int(misaligned), k])
	region = SEED_VECS * vec
	nan = np.uint32(tn.NAN_POS32) if dtype == F32 else np.uint16(tn.NAN_POS32 >> 16)
	ninf = _to_bits([np.float32(-np.inf)], dtype)[0]
	rows = []
	for j in range(Q):
		n = k - 1 if j % 2 else (2, k // 2, k - 1, 3)[(j // 2) % 4]
		row = np.full(I, ninf if j % 2 else nan)
		vals = _distinct_rows(rng, 1, I, dtype)[0][:n]
		g = rng.choice(np.arange(2, SEED_VECS - 2, 2), size=2, replace=False)
		pos = np.concatenate([vec + g * vec + rng.integers(vec, size=2), rng.choice(np.arange(region + vec, I), size=n - 2, replace=False)])
		row[pos] = vals
		if j % 4 == 0:
			row[int(rng.integers(region + vec, I))] = ninf       # one -inf among the NaN row's numbers (it may overwrite one of them)
		rows.append(row)
	pred = _check(ops, gpu, rows, dtype, misaligned, lambda kk: (2, 2), "short rows", ks=(k,))
	assert pred[k] == (Q, Q)


# ------------------------------------------------------------------ 7: the entry with counters, captured into a graph and replayed
@pytest.mark.parametrize("dtype", [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")])
def test_capture_and_replay_adds_to_the_counters(ops, gpu, auto_rank, dtype):
	"""anncur_rowwise_topk_ex keeps the stream contract with a counter pointer too: captured once (nothing runs, the counters stay zero), every
	replay gives the reference's rows in freshly poisoned outputs and adds the predicted counts once more."""
	I, k = 40000, 100
	rng = np.random.default_rng([7, VEC[dtype]])
	rows = _distinct_rows(rng, Q, I, dtype)
	rank = auto_rank(I, k, dtype)
	for j in range(1, Q, 2):
		_plant_best_in_seed(rng, rows[j], dtype, rank + 3, VEC[dtype])
	A, _buf = _poisoned_view(rows, I, dtype, True, gpu)
	started, restarted = _predict_rows(rows, dtype, k, rank, _heads(A))
	assert started == Q and 0 < restarted < Q
	want_v, want_i = _reference(rows, dtype)
	val = torch.empty((Q, k), dtype=torch.float32, device=gpu)
	idx = torch.empty((Q, k), dtype=torch.int32, device=gpu)
	stats = torch.zeros(2, dtype=torch.int32, device=gpu)
	ops.rowwise_topk(A, k, out=(val, idx), _stats=stats)          # (eagerly once: nothing is set up for the first time inside the capture)
	torch.cuda.synchronize()
	assert stats.cpu().tolist() == [restarted, started]
	stats.zero_()
	torch.cuda.synchronize()
	g = torch.cuda.CUDAGraph()
	with torch.cuda.graph(g, capture_error_mode="thread_local"):
		got = ops.rowwise_topk(A, k, out=(val, idx), _stats=stats)
	torch.cuda.synchronize()
	assert stats.cpu().tolist() == [0, 0]
	for n in (1, 2, 3):
		val.fill_(float("nan")); idx.fill_(-7)
		torch.cuda.synchronize()
		g.replay()
		torch.cuda.synchronize()
		_assert_same(got, want_v[:, :k], want_i[:, :k], f"replay {n}")
		assert stats.cpu().tolist() == [n * restarted, n * started]
