"""anncur_overlap_counts (both kernels), ops.overlap_counts' chunking and mapped_host_out, ops.copy_to_mapped_host and the closed form of
retrieval.overlap_cells / overlap_pool_cells, each held to equality with a plain reference (tests/overlap_numpy.py: Python sets;
tests/topk_numpy.py for the chain).  DESIGN 4.3a names, for every branch of the kernels, the test here that enters it.

Q = 7 unless a test is about Q: not a multiple of 4, so the wave kernel runs two workgroups and the second has an idle wave."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_numpy as tn  # noqa: E402
from overlap_numpy import first_pos, overlap_ref  # noqa: E402

pytestmark = pytest.mark.gpu

Q7 = 7
BIG = 2 ** 31 - 1
MIN = -2 ** 31
FRESH = 1 << 30       # ids from here up to BIG - 1 are in no universe below: free to overwrite an entry with
POISON = 0x5a5a5a5a
WAVE_SIZES = (1, 63, 64, 65, 127, 128)
LONG_SIZES = ((129, 1), (1, 129), (128, 129), (129, 128), (255, 257), (256, 256), (257, 255), (4096, 4096), (4096, 1), (1, 4096))
FOUR_SIZES = ((40, 100), (100, 40), (128, 128), (300, 700))


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _dev(x):
	x = np.asarray(x)
	assert x.size == 0 or (x.min() >= MIN and x.max() <= BIG)
	return torch.from_numpy(np.array(x, dtype=np.int32, order="C")).cuda()


def _poison_next_allocation(shape):
	"""ops.overlap_counts allocates its own device result: leave a poisoned block of that size in torch's caching allocator, so that a
	row the kernel does not write does not come back holding the right counts of an earlier call."""
	if int(np.prod(shape)):
		t = torch.full(shape, POISON, dtype=torch.int32, device="cuda")
		torch.cuda.synchronize()
		del t


def _counts(ops, a, b, pairs):
	_poison_next_allocation((len(pairs), a.shape[0]))
	out = ops.overlap_counts(_dev(a), _dev(b), pairs)
	assert out.dtype == torch.int32 and tuple(out.shape) == (len(pairs), a.shape[0]) and out.is_cuda
	return out.cpu().numpy()


def _check(ops, a, b, pairs):
	got, want = _counts(ops, a, b, pairs), overlap_ref(a, b, pairs)
	bad = np.argwhere(got != want)
	assert bad.size == 0, [(pairs[p], int(q), int(got[p, q]), int(want[p, q])) for p, q in bad[:8]]
	return got


def _universe(rng, n):
	"""n distinct ids in 1 .. 2^30 - 1, in random order."""
	u = np.unique(rng.integers(1, FRESH, size=n + 64))
	assert u.size >= n
	return rng.permutation(u)[:n].astype(np.int64)


def _plant(rng, row, ids):
	"""Overwrite len(ids) random positions of row (fewer if it is shorter) with ids."""
	pos = rng.choice(row.size, size=min(len(ids), row.size), replace=False)
	row[pos] = ids[:pos.size]


def _distinct_rows(rng, Q, la, lb, plant=True):
	"""a [Q x la], b [Q x lb] (int64 values in int32 range): ids distinct within a row, no pads, about half of a's ids in b where the sizes
	allow it (the universe holds 2 lb ids, or la if that is more); id 0 and id 2^31 - 1 in both lists (one of them in a list of one)."""
	a, b = np.empty((Q, la), dtype=np.int64), np.empty((Q, lb), dtype=np.int64)
	for q in range(Q):
		u = _universe(rng, max(2 * lb, la) + 2)
		a[q], b[q] = rng.choice(u, la, replace=False), rng.choice(u, lb, replace=False)
		if plant:
			edge = [0, BIG] if q % 2 == 0 else [BIG, 0]
			_plant(rng, a[q], edge)
			_plant(rng, b[q], edge if q % 4 < 2 else edge[::-1])
	return a, b


def _random_pairs(rng, la, lb, n):
	return [(int(rng.integers(0, la + 1)), int(rng.integers(0, lb + 1))) for _ in range(n)]


def _distinct_pairs(rng, la, lb, n):
	cell = rng.choice((la + 1) * (lb + 1), size=n, replace=False)
	return [(int(c) // (lb + 1), int(c) % (lb + 1)) for c in cell]


# ------------------------------------------------------------------ A. sizes: distinct ids, no pads
def _size_case(la, lb):
	rng = np.random.default_rng(1000 * la + lb)
	a, b = _distinct_rows(rng, Q7, la, lb)
	return a, b, [(0, lb), (la, 0), (la, lb), (1, 1), (la, 1), (1, lb)] + _random_pairs(rng, la, lb, 6)


@pytest.mark.parametrize("lb", WAVE_SIZES)
@pytest.mark.parametrize("la", WAVE_SIZES)
def test_sizes_on_the_wave_kernel(ops, la, lb):
	a, b, pairs = _size_case(la, lb)
	got = _check(ops, a, b, pairs)
	assert (got[0] == 0).all() and (got[1] == 0).all() and got[2].max() >= 1       # empty prefixes; 0 or 2^31 - 1 is found at full length


@pytest.mark.parametrize("la,lb", LONG_SIZES)
def test_sizes_on_the_long_kernel(ops, la, lb):
	a, b, pairs = _size_case(la, lb)
	got = _check(ops, a, b, pairs)
	assert (got[0] == 0).all() and (got[1] == 0).all() and got[2].max() >= 1


# ------------------------------------------------------------------ B. pads and other negative ids
def _pad_case(la, lb):
	"""About 20 % of each list is -1; row 2 of a and row 4 of b are pads only; 0, 2^31 - 1, -2 and -2^31 stand in both lists of every other
	row within the first 11 positions (so the pair (11, 11) has the negative ids inside both prefixes)."""
	rng = np.random.default_rng(2000 * la + lb)
	a, b = _distinct_rows(rng, Q7, la, lb, plant=False)
	a[rng.random(a.shape) < 0.2] = -1
	b[rng.random(b.shape) < 0.2] = -1
	for q in range(Q7):
		a[q, q:q + 4] = [0, -2, MIN, BIG]
		b[q, q + 1:q + 5] = [MIN, BIG, -2, 0]
	a[2], b[4] = -1, -1
	pairs = [(la, lb), (0, lb), (la, 0), (11, 11), (la, 11), (11, lb)] + _random_pairs(rng, la, lb, 6)
	return a, b, pairs


@pytest.mark.parametrize("la,lb", FOUR_SIZES)
def test_pads_and_negative_ids_are_in_no_set(ops, la, lb):
	a, b, pairs = _pad_case(la, lb)
	assert abs((a == -1).mean() - 0.2) < 0.2 and (a[2] == -1).all() and (b[4] == -1).all()
	got = _check(ops, a, b, pairs)
	assert (got[:, 2] == 0).all() and (got[:, 4] == 0).all()
	# (11, 11): of the four planted ids only 0 and 2^31 - 1 may count -- and they do, in every row but the two pad rows
	rows = [q for q in range(Q7) if q not in (2, 4)]
	for q in rows:
		assert {-2, MIN} <= set(a[q, :11].tolist()) & set(b[q, :11].tolist())
	assert (got[3, rows] >= 2).all()


@pytest.mark.parametrize("width", [5, 129])
def test_a_negative_id_in_both_prefixes_adds_nothing(ops, width):
	"""By hand, on both kernels (width 129: the same rows padded with -1)."""
	row = [-1, -2, MIN, 5, 6] + [-1] * (width - 5)
	a = np.array([row, row[::-1][:width]], dtype=np.int64)
	b = np.array([row, row], dtype=np.int64)
	got = _check(ops, a, b, [(3, 3), (4, 4), (5, 5), (width, width)])
	assert got[:, 0].tolist() == [0, 1, 2, 2] and got[3, 1] == 2


# ------------------------------------------------------------------ C. repeated ids in b
def _b_repeats_case(la, lb):
	"""a distinct, b drawn with replacement.  Row q also gets one planted id x = a[q, ja] whose only positions in b are p < p2.
	-> a, b, pairs, plants [(q, p, p2)].  The plants put p and p2 in the same and in different halves of 64, with x in either half of a."""
	rng = np.random.default_rng(3000 * la + lb)
	want_plants = [(5, 10, 70), (100, 10, 70), (70, 3, 40), (5, 70, 100), (0, 0, 1), (la - 1, lb - 2, lb - 1), (la - 1, 0, lb - 1)]
	a, b = np.empty((Q7, la), dtype=np.int64), np.empty((Q7, lb), dtype=np.int64)
	pairs, plants = [(la, lb), (la, 0)], []
	for q in range(Q7):
		u = _universe(rng, max(la, lb) + 8)
		a[q] = rng.choice(u, la, replace=False)
		b[q] = rng.choice(u, lb, replace=True)
		ja, p, p2 = want_plants[q]
		if not (ja < la and p < p2 < lb):
			ja, p, p2 = min(ja, la - 1), p % (lb // 2), lb // 2 + p2 % (lb // 2)
		x = a[q, ja]
		hit = np.flatnonzero(b[q] == x)
		b[q, hit] = FRESH + q * 4096 + np.arange(hit.size)
		b[q, [p, p2]] = x
		free_a = [j for j in range(la) if j != ja]
		a[q, rng.choice(free_a, 2, replace=False)] = [0, BIG]
		free_b = [t for t in range(lb) if t not in (p, p2)]
		b[q, rng.choice(free_b, 2, replace=False)] = [BIG, 0]
		assert first_pos(b[q], x) == p and np.flatnonzero(b[q] == x).tolist() == [p, p2]
		plants.append((q, p, p2))
		pairs += [(la, p), (la, p + 1), (la, p2), (la, p2 + 1)]
	pairs += _random_pairs(rng, la, lb, 6)
	return a, b, pairs, plants


@pytest.mark.parametrize("la,lb", FOUR_SIZES)
def test_repeated_ids_in_b_count_at_their_first_position(ops, la, lb):
	a, b, pairs, plants = _b_repeats_case(la, lb)
	assert all(np.unique(a[q]).size == la for q in range(Q7)) and any(np.unique(b[q]).size < lb for q in range(Q7))
	got = _check(ops, a, b, pairs)
	for q, p, p2 in plants:
		c = {kb: int(got[pairs.index((la, kb)), q]) for kb in (p, p + 1, p2, p2 + 1)}
		assert c[p + 1] == c[p] + 1 and c[p2 + 1] == c[p2], (q, p, p2, c)      # position p holds the planted id and nothing else: +1 there, +0 at p2


@pytest.mark.parametrize("k_retvr", [60, 100])       # the pool is 97 ids (wave kernel) or 137 (long kernel)
def test_pool_list_that_names_three_anchors_again(ops, k_retvr):
	from anncur_amd import retrieval as R
	rng = np.random.default_rng(k_retvr)
	u = _universe(rng, 400)
	anchors, rest = u[:37].copy(), u[37:]
	anchors[[3, 20]] = [0, BIG]
	retrieved = np.stack([rng.choice(rest, k_retvr, replace=False) for _ in range(Q7)])
	retrieved[:, [0, k_retvr // 2, k_retvr - 1]] = anchors[[5, 20, 36]]
	exact = np.stack([rng.permutation(np.concatenate([anchors[[5, 20, 36, 1]], rng.choice(rest, 46, replace=False)])) for _ in range(Q7)])
	pool = R.pool_list(anchors, _dev(retrieved))
	assert tuple(pool.shape) == (Q7, 37 + k_retvr)
	cells = [(1, 10), (10, k_retvr), (50, k_retvr), (50, 0), (50, 1), (50, k_retvr // 2 + 1)]
	pairs = R.pool_pairs(cells, 37)
	got = _check(ops, exact, pool.cpu().numpy(), pairs)
	want = [[len(set(exact[q, :k].tolist()) & (set(anchors.tolist()) | set(retrieved[q, :kr].tolist()))) for q in range(Q7)] for k, kr in cells]
	assert got.tolist() == want and (got[3] == 4).all() and np.array_equal(got[3], got[4])      # the anchors named again add nothing


# ------------------------------------------------------------------ D. repeated ids in a
def _a_repeats_case(la, lb):
	rng = np.random.default_rng(4000 * la + lb)
	a, b = np.empty((Q7, la), dtype=np.int64), np.empty((Q7, lb), dtype=np.int64)
	for q in range(Q7):
		u = _universe(rng, max(la, 4))
		u[:2] = [0, BIG]
		a[q] = rng.choice(u[:max(la // 2, 2)], la, replace=True)       # every id of a about twice
		b[q] = rng.choice(u, lb, replace=True)
		_plant(rng, a[q], [0, BIG] if la > 3 else [0])
		_plant(rng, b[q], [BIG, 0])
	pairs = [(la, lb), (la, 1), (1, lb), (min(64, la), lb), (min(65, la), lb), (la, min(64, lb)), (la, min(65, lb))] + _random_pairs(rng, la, lb, 8)
	return a, b, pairs


@pytest.mark.parametrize("la,lb", [(3, 3), (65, 2), (128, 128), (129, 128), (300, 700)])
def test_repeated_ids_in_a_count_once(ops, la, lb):
	a, b, pairs = _a_repeats_case(la, lb)
	assert any(np.unique(a[q]).size < la for q in range(Q7))
	if (la, lb) == (3, 3):
		a[0], b[0] = [5, 5, 7], [5, 9, 9]
	if la >= 65:
		x = FRESH + 1                                          # a[0] == a[64]: the same id in both halves of a wave's a
		a[0][a[0] == x] = FRESH + 2
		a[0, [0, 64]], b[0, 0] = x, x
		y = FRESH + 3                                          # an id repeated inside the second half only
		a[1][a[1] == y] = FRESH + 2
		a[1, [la - 1, 64 + (la - 65) // 2]], b[1, lb - 1] = y, y
	got = _check(ops, a, b, pairs)
	if (la, lb) == (3, 3):
		assert got[0, 0] == 1
	if la >= 65:
		full, to64, to65 = (got[pairs.index(p)] for p in ((la, lb), (64, lb), (65, lb)))
		assert to65[0] == to64[0] and full[1] >= 1             # a[64] repeats a[0]: the 65th entry adds nothing


@pytest.mark.parametrize("width", [3, 129])
def test_repeated_ids_in_a_by_hand(ops, width):
	"""The two kernels disagreed on these before both were held to the set formula (width 129: the same rows, -1 padded, on the long kernel)."""
	pad = [-1] * (width - 3)
	a = np.array([[5, 5, 7] + pad, [7, 5, 5] + pad, [5, 5, 5] + pad, [9, 5, 9] + pad], dtype=np.int64)
	b = np.array([[5, 9, 9] + pad] * 4, dtype=np.int64)
	got = _check(ops, a, b, [(3, 3), (2, 3), (1, 3), (3, 1), (3, 2)])
	assert got.tolist() == [[1, 1, 1, 2], [1, 1, 1, 2], [1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 2]]


def test_counts_do_not_depend_on_the_route(ops):
	"""The same a and b at (128, 128), wave kernel, and with one more column of b, long kernel, under pairs that leave that column out:
	repeats in both lists and pads."""
	rng = np.random.default_rng(77)
	u = _universe(rng, 90)
	a, b = rng.choice(u, (Q7, 128), replace=True), rng.choice(u, (Q7, 128), replace=True)
	a[rng.random(a.shape) < 0.1] = -1
	b[rng.random(b.shape) < 0.1] = -1
	a[:, 64] = a[:, 0]
	a[0, [0, 64]], b[0, [3, 90]] = FRESH + 1, FRESH + 1
	pairs = [(128, 128), (65, 128), (64, 128), (128, 64), (128, 65), (1, 128)] + _random_pairs(rng, 128, 128, 10)
	wave = _check(ops, a, b, pairs)
	for extra in (a[:, 0], np.full(Q7, -1), u[rng.integers(0, 90, Q7)]):
		assert np.array_equal(_check(ops, a, np.concatenate([b, extra[:, None]], axis=1), pairs), wave)
	a129 = np.concatenate([a, a[:, :1]], axis=1)           # and with one more column of a, which repeats a[:, 0]
	assert np.array_equal(_check(ops, a129, b, pairs), wave)
	assert np.array_equal(_check(ops, a129, b, [(129, kb) for _, kb in pairs]), _check(ops, a, b, [(128, kb) for _, kb in pairs]))


# ------------------------------------------------------------------ E. pairs: the 64 per launch and the chunks of ops
def _pairs_case(lb, n_pairs):
	rng = np.random.default_rng(5000 + lb + n_pairs)
	a, b = _distinct_rows(rng, Q7, 100, lb)
	return a, b, _distinct_pairs(rng, 100, lb, n_pairs)


@pytest.mark.parametrize("lb", [100, 200])             # wave kernel, long kernel
@pytest.mark.parametrize("n_pairs", [1, 64, 65, 130])
def test_pair_counts_and_chunk_offsets(ops, n_pairs, lb):
	a, b, pairs = _pairs_case(lb, n_pairs)
	assert len(set(pairs)) == n_pairs
	got = _check(ops, a, b, pairs)
	if n_pairs == 130:
		assert not np.array_equal(got[0:64], got[64:128]) and not np.array_equal(got[0:2], got[128:130])


@pytest.mark.parametrize("lb", [100, 200])
def test_no_pairs_and_no_queries(ops, lb):
	rng = np.random.default_rng(lb)
	a, b = _distinct_rows(rng, Q7, 100, lb)
	out = ops.overlap_counts(_dev(a), _dev(b), [])
	assert tuple(out.shape) == (0, Q7) and out.dtype == torch.int32
	for n_pairs in (1, 65):
		out = ops.overlap_counts(_dev(a[:0]), _dev(b[:0]), _distinct_pairs(rng, 100, lb, n_pairs))
		assert tuple(out.shape) == (n_pairs, 0) and out.dtype == torch.int32
	torch.cuda.synchronize()


# ------------------------------------------------------------------ F. Q
@pytest.mark.parametrize("Q,lb", [(1, 100), (3, 100), (4, 100), (5, 100), (1000, 100), (1, 200), (1000, 200)])
def test_query_counts(ops, Q, lb):
	rng = np.random.default_rng(6000 + Q + lb)
	a, b = _distinct_rows(rng, Q, 100, lb)
	got = _check(ops, a, b, [(100, lb), (10, lb), (100, 10)] + _random_pairs(rng, 100, lb, 3))
	assert Q < 1000 or np.unique(got[0]).size > 5


# ------------------------------------------------------------------ G. mapped_host_out
def _pinned(shape, dtype=torch.int32):
	return torch.empty(shape, dtype=dtype, pin_memory=True)


_MAPPED_CASES = [("pads", s) for s in FOUR_SIZES] + [("b_repeats", s) for s in FOUR_SIZES] + [("pairs130", (100, 100)), ("pairs130", (100, 200))]


@pytest.mark.parametrize("kind,size", _MAPPED_CASES)
def test_mapped_host_out_receives_the_same_counts(ops, kind, size):
	if kind == "pads":
		a, b, pairs = _pad_case(*size)
	elif kind == "b_repeats":
		a, b, pairs = _b_repeats_case(*size)[:3]
	else:
		a, b, pairs = _pairs_case(size[1], 130)
	host = _pinned((len(pairs), Q7))
	host.fill_(POISON)
	assert host.is_pinned() and (host == POISON).all()
	ret = ops.overlap_counts(_dev(a), _dev(b), pairs, mapped_host_out=host)
	torch.cuda.synchronize()
	assert ret is host
	got, want = host.numpy().copy(), overlap_ref(a, b, pairs)
	bad = np.argwhere(got != want)
	assert bad.size == 0, [(int(p), pairs[p], int(q), hex(int(got[p, q]) & 0xffffffff), int(want[p, q])) for p, q in bad[:8]]
	assert np.array_equal(got, _counts(ops, a, b, pairs))


def test_mapped_host_arguments_are_validated(ops):
	"""The checks that need a PINNED tensor (the unpinned one: tests/test_cpu_overlap_host.py).  Nothing is launched, nothing written."""
	a, b = _dev(np.arange(70).reshape(7, 10)), _dev(np.arange(140).reshape(7, 20))
	pairs = [(1, 1), (2, 2)]
	msg = "contiguous pinned int32 host tensor"
	for bad in (_pinned((2, 7), torch.int64), _pinned((2, 7), torch.float32), _pinned((7, 2)), _pinned((2, 8)), _pinned((3, 7)), _pinned((14,)),
				_pinned((7, 2)).t(), _pinned((2, 14))[:, ::2], torch.empty((2, 7), dtype=torch.int32), torch.empty((2, 7), dtype=torch.int32, device="cuda")):
		if not bad.is_cuda:
			bad.fill_(7)
		with pytest.raises(ValueError, match=msg):
			ops.overlap_counts(a, b, pairs, mapped_host_out=bad)
		assert bad.is_cuda or (bad == 7).all()
	with pytest.raises(ValueError, match=msg):
		ops.overlap_counts(a, b, [], mapped_host_out=_pinned((2, 7)))
	src = torch.arange(64, dtype=torch.uint8, device="cuda")
	for dst in (_pinned((63,), torch.uint8), _pinned((65,), torch.uint8), _pinned((15,), torch.int32), _pinned((8, 9), torch.uint8)):
		with pytest.raises(ValueError, match="size mismatch"):
			ops.copy_to_mapped_host(src, dst)
	for dst in (torch.empty(64, dtype=torch.uint8), torch.empty(64, dtype=torch.uint8, device="cuda"), _pinned((64, 2), torch.uint8)[:, 0]):
		with pytest.raises(ValueError, match="contiguous pinned host tensor"):
			ops.copy_to_mapped_host(src, dst)
	torch.cuda.synchronize()


# ------------------------------------------------------------------ H. copy_to_mapped_host
GUARD = 256
GUARD_BYTE = 0xA5


def _window(nbytes):
	"""A 16-byte-aligned contiguous window of nbytes inside a larger pinned tensor of guard bytes."""
	whole = _pinned((nbytes + 2 * GUARD,), torch.uint8)
	whole.fill_(GUARD_BYTE)
	win = whole[GUARD:GUARD + nbytes]
	if not win.is_pinned():
		pytest.skip("a view into a pinned tensor does not report is_pinned() here: copy_to_mapped_host refuses it")
	assert win.is_contiguous() and win.data_ptr() % 16 == 0
	return whole, win


def _check_copy(ops, src, nbytes):
	before = src.cpu()
	whole, win = _window(nbytes)
	assert ops.copy_to_mapped_host(src, win) is None
	torch.cuda.synchronize()
	want = before.contiguous().view(torch.uint8).reshape(-1) if nbytes else torch.empty(0, dtype=torch.uint8)
	assert torch.equal(whole[GUARD:GUARD + nbytes], want)
	assert (whole[:GUARD] == GUARD_BYTE).all() and (whole[GUARD + nbytes:] == GUARD_BYTE).all()
	assert torch.equal(src.cpu(), before)


@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4095, 4096, 4097, 256 * 16, 257 * 16, 4096 * 16 + 7, (1 << 20) + 3])
def test_copy_to_mapped_host_bytes(ops, nbytes):
	src = ((torch.arange(nbytes, dtype=torch.int64) * 7 + 3) % 251).to(torch.uint8).cuda()      # a counter: a shifted or repeated block shows
	_check_copy(ops, src, nbytes)


def test_copy_to_mapped_host_other_dtypes(ops):
	_check_copy(ops, (torch.arange(33 * 7, dtype=torch.int32) * 2654435 - 300000000).reshape(33, 7).cuda(), 33 * 7 * 4)       # 924 bytes: 57 x 16 + 12
	_check_copy(ops, (torch.arange(65, dtype=torch.float32) - 30).to(torch.bfloat16).reshape(5, 13).cuda(), 130)
	_check_copy(ops, torch.arange(40, dtype=torch.int32).reshape(4, 10).cuda()[:, ::2], 80)                                    # a strided source is copied row-major


def test_copy_of_zero_bytes_writes_nothing(ops):
	from anncur_amd import _lib
	whole, win = _window(64)
	src = torch.arange(64, dtype=torch.uint8, device="cuda")
	if win[:0].is_pinned():                                  # (an empty view has no data pointer to ask about: torch may call it pageable)
		assert ops.copy_to_mapped_host(src[:0], win[:0]) is None
	assert _lib.load().anncur_copy_bytes(ops._p(src), ops._p(win), 0, ops._stream()) == 0
	torch.cuda.synchronize()
	assert (whole == GUARD_BYTE).all()


# ------------------------------------------------------------------ I. the chain on tie-heavy data
TOP_KS = (1, 10, 50, 100)
K_RETVRS = (100, 128, 129, 500)
CELLS = [(k, kr) for kr in K_RETVRS for k in TOP_KS]
N_ANC = 37


@pytest.fixture(scope="module")
def chain():
	"""A: 8 x 3001 quarters in [-2, 2] (17 values, ~176 items each: every k-th place lies inside a tie; no negative zero), S = A + noise on
	the same grid.  Row 3 of A keeps 60 scores (the rest NaN: exact rows end in pads), row 5 of S keeps 110 (retrieved rows end in pads).
	The reference lists are computed here once and only read by the tests."""
	rng = np.random.default_rng(2024)
	Q, I = 8, 3001
	A = (rng.integers(-8, 9, (Q, I)) / 4).astype(np.float32)
	S = (A + rng.integers(-2, 3, (Q, I)) / 4).astype(np.float32)
	assert not np.signbit(A[A == 0]).any() and not np.signbit(S[S == 0]).any()
	A[3, rng.permutation(I)[60:]] = np.nan
	S[5, rng.permutation(I)[110:]] = np.nan
	anchors = np.sort(rng.choice(I, N_ANC, replace=False))
	S_wo = S.copy()
	S_wo[:, anchors] = np.nan                               # a retrieval with the anchors excluded
	ref = {"exact": np.stack([tn.topk_ref(A[q], 100)[1] for q in range(Q)]),
		   "approx": np.stack([tn.topk_ref(S[q], 500)[1] for q in range(Q)]),
		   "new": np.stack([tn.topk_ref(S_wo[q], 500)[1] for q in range(Q)])}
	for v in ref.values():
		v.setflags(write=False)
	return {"A": A, "S": S, "anchors": anchors, "Q": Q, **ref}


def _valid(ids):
	return {int(x) for x in ids if x >= 0}


def _loop_counts(chain, cand_of):
	"""[n_cells, Q]: |exact[:k] & rerank(cand_of(q, kr))[:k]| from topk_ref and rerank_ref, one query and one cell at a time."""
	out = np.zeros((len(CELLS), chain["Q"]), dtype=np.int32)
	for j, (k, kr) in enumerate(CELLS):
		for q in range(chain["Q"]):
			ex = tn.topk_ref(chain["A"][q], k)[1]
			rr = tn.rerank_ref(chain["A"][q], cand_of(q, kr), k)[1]
			out[j, q] = len(_valid(ex) & _valid(rr))
	return out


def test_chain_closed_form_literal_rerank_and_loop_agree(ops, chain):
	from anncur_amd import retrieval as R
	A_dev = torch.from_numpy(chain["A"]).cuda()
	exact, approx = ops.rowwise_topk(A_dev, 100), ops.rowwise_topk(torch.from_numpy(chain["S"]).cuda(), 500)
	assert np.array_equal(exact.indices.cpu().numpy(), chain["exact"]) and np.array_equal(approx.indices.cpu().numpy(), chain["approx"])
	assert (chain["exact"][3, 60:] == -1).all() and (chain["approx"][5, 110:] == -1).all()
	want = _loop_counts(chain, lambda q, kr: chain["approx"][q, :kr])
	closed = R.overlap_cells(exact.indices, approx.indices, CELLS).cpu().numpy()
	literal = R.overlap_cells(exact.indices, approx.indices, CELLS, A_dev, literal_rerank=True).cpu().numpy()
	assert np.array_equal(closed, want), np.argwhere(closed != want)[:8]
	assert np.array_equal(literal, want), np.argwhere(literal != want)[:8]
	assert np.array_equal(want, overlap_ref(chain["exact"], chain["approx"], CELLS))
	# the same cells from a retrieved list of 128: the closed form on the wave kernel
	short = [c for c in CELLS if c[1] <= 128]
	got = R.overlap_cells(exact.indices, approx.indices[:, :128].contiguous(), short).cpu().numpy()
	assert np.array_equal(got, want[[CELLS.index(c) for c in short]])
	assert want[CELLS.index((100, 500)), 3] <= 60 and (want[CELLS.index((1, 100))] <= 1).all() and want.max() > 10


def _placeholders(ids, base):
	"""A list for compute_overlap, which counts plain Python-set members: each -1 pad becomes a negative id of its own (the list keeps its
	length, the pads meet nothing)."""
	return [int(x) if x >= 0 else base - j for j, x in enumerate(ids)]


@pytest.mark.parametrize("literal", [False, True])
def test_eval_topk_recall_equals_compute_overlap_of_the_lists(ops, chain, literal):
	from anncur_amd import retrieval as R
	from anncur_amd.eval_utils import compute_overlap, flatten_overlap
	A_dev = torch.from_numpy(chain["A"]).cuda()
	approx_idx = _dev(chain["approx"])
	subsets = {"anchor": [0, 3, 5], "non_anchor": [1, 2, 4, 6, 7], "all": list(range(8))}

	def lists(k, kr, rows):
		l1 = [_placeholders(tn.topk_ref(chain["A"][q], k)[1], -10) for q in rows]
		l2 = [_placeholders(tn.rerank_ref(chain["A"][q], chain["approx"][q, :kr], k)[1], -10000) for q in rows]
		return l1, l2
	got = R.eval_topk_recall(A_dev, approx_idx, TOP_KS, K_RETVRS, literal_rerank=literal)
	got_sub = R.eval_topk_recall(A_dev, approx_idx, TOP_KS, K_RETVRS, row_subsets=subsets, literal_rerank=literal)
	assert sorted(got) == sorted(got_sub) == sorted(CELLS)
	for k, kr in CELLS:
		assert got[(k, kr)] == flatten_overlap(compute_overlap(*lists(k, kr, range(8)))), (k, kr)
		assert got_sub[(k, kr)] == {name: flatten_overlap(compute_overlap(*lists(k, kr, rows))) for name, rows in subsets.items()}, (k, kr)


def test_pool_cells_closed_form(ops, chain):
	from anncur_amd import retrieval as R
	anchors, Q = chain["anchors"], chain["Q"]
	exact_idx = _dev(chain["exact"])
	assert not np.isin(chain["new"], anchors).any() and np.isin(chain["approx"], anchors).any()
	for retrieved in (chain["new"], chain["approx"]):      # the anchors excluded from the retrieval, and not: the list then names some twice
		pool_of = lambda q, kr: np.concatenate([anchors, retrieved[q, :kr]])
		want = np.array([[len(_valid(chain["exact"][q, :k]) & _valid(pool_of(q, kr))) for q in range(Q)] for k, kr in CELLS])
		if retrieved is chain["new"]:                       # a pool without repeats: the re-rank loop is defined, and says the same
			assert np.array_equal(_loop_counts(chain, pool_of), want)
		got = R.overlap_pool_cells(exact_idx, anchors, _dev(retrieved), CELLS).cpu().numpy()
		assert np.array_equal(got, want), np.argwhere(got != want)[:8]
	# 37 anchors + 60 retrieved: the pool on the wave kernel
	cells = [(k, kr) for kr in (10, 60, 91) for k in TOP_KS]
	got = R.overlap_pool_cells(exact_idx, anchors, _dev(chain["approx"][:, :91]), cells).cpu().numpy()
	want = [[len(_valid(chain["exact"][q, :k]) & _valid(np.concatenate([anchors, chain["approx"][q, :kr]]))) for q in range(Q)] for k, kr in cells]
	assert got.tolist() == want
