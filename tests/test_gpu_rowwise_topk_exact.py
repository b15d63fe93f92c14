"""Exact-data tests of the row-wise top-k family of csrc/topk.hip (wave_select.hpp, select.hpp) against plain numpy on the host
(tests/topk_numpy.py): anncur_rowwise_topk (short-row, wave-per-row and workgroup kernels), anncur_rowwise_topk_ragged,
anncur_rowwise_topk_gather and anncur_rerank.

Nothing here has a tolerance: values are compared as bit patterns, indices exactly.  The order is defined (score descending, then the
smaller index; NaN never selected; -inf an ordinary candidate; (-inf, -1) padding), the data is built from integer bit patterns, and -0.0
is kept out of every part but E -- so the reference's answer is the only one.

Every matrix is an interior view of a larger buffer whose every other element is POISON (+inf, NaN, 3e38 in turn): the margin rows and
columns, the pitch pad, and in the ragged launches everything behind a row's length.  A read outside a row's [start, start + length)
therefore stays inside the test's own allocation and wins the top-k.  Nothing here tries to observe a read outside an allocation.

  A  ragged rows: every length at which the wave kernel takes another path (wave step, seed threshold, the clamp-free block loop's first
     and second turn), for aligned rows and for rows whose 16-byte grid starts at every possible head, k on both sides of the one-key /
     two-key final sort; distinct data, tie-heavy data, constant / -inf / NaN rows.
  B  whole 16-byte vectors of NaN inside the 512 vectors the wave kernel seeds its threshold from.  fp32 maxima of four NaNs used to keep
     their NaN pattern, and with the sign bit clear that pattern's sortable key lies above every number's: m such vectors counted as the m
     largest group maxima, the seed became the (k - m)-th largest real maximum -- no lower bound on the k-th best -- and the row came back
     short.  Fixed with this file (ScanPre<float>::group_max_key: a NaN maximum keys 0, as in the bf16 version).
  C  the workgroup scan (k = 129 .. 2048): sizes around its trigger check (2048 elements) and one turn of its four prefetch sets (8192),
     I = k, misaligned rows (head and tail are offered BEFORE the stream, so the largest indices come first and must lose the ties).
  D  re-rank: k_retvr and k_out on both sides of every kernel class and of the 256-thread step, holes among the candidates, an id pitch
     wider than k_retvr.
  E  denormals (the keys are bit-ordered; a float compare that flushed would tie them all) and zeros of both signs (their
     mutual order is unspecified, everything else about such a row is not).

Against the parent of the commit that added this file (same tests, the library without the fix), on an MI355X: the three fp32 cases of B
with sign-clear NaNs fail as predicted -- see test_nan_vectors_in_the_seed_region's docstring -- and the other 78 tests pass.

Mutations tried on scratch builds of the library when this file was written (81 tests, 3.8 s on an MI355X), each run once:
  * the ragged launch ignores row_len (every row is scanned to I_max; the reads stay inside the matrix): all 20 test_ragged_rows cases and
    all 12 of test_nan_vectors_in_the_seed_region fail (its ragged launches mix four lengths) -- the poison wins.
  * the wave kernel's drain pushes `idx` instead of `0xffffffff - idx` as the low key half: the same 32 fail, and test_denormals_keep_their_order
    and test_zeros_of_both_signs_around_the_kth_place at k = 64 (36 in all): every index that went through the stream's drain is wrong, ties or not.
  * sel_offer's float prefilter as `v > tau` (an element that ties with the threshold's score no longer reaches the key compare): all 8
    test_workgroup_scan cases fail and nothing else.  In every launch the mostly -inf rows come back short (-inf never beats the initial
    -inf), and in the misaligned launches every _tail_threshold_row with a tail fails (6 of 8 rows for fp32): the tail is offered first, a
    compaction makes one of ITS elements the k-th kept key, and the stream's equal scores with smaller indices are turned away.  The tie
    alphabet and the constant rows do NOT notice this mutant: there a compaction never keeps a tail element (among equal scores the tail's
    indices are the largest), so every later tie loses under either compare -- which is why the rows above were built.
  * sel_offer's key compare as `key >= tau_key`: SURVIVES, and should -- the keys of a row are distinct and every element is offered once, so
    no offered key ever equals the threshold key (the k-th kept key, an element already in the buffer).  An equivalent mutant.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
VEC = {F32: 4, BF16: 8}
NEG_INF32 = np.float32(-np.inf)


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


# ------------------------------------------------------------------ bits <-> tensors, the poisoned buffer
def _bits_dtype(dtype):
	return np.uint32 if dtype == F32 else np.uint16


def _to_bits(values, dtype):
	"""float32 values (exactly representable in `dtype`) -> the element type's bit patterns."""
	v = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
	return v.view(np.uint32).copy() if dtype == F32 else tn.f32_to_bf16_bits(v)


def _to_f32(bits, dtype):
	return tn.f32_from_bits(bits) if dtype == F32 else tn.bf16_bits_to_f32(bits)


def _poisoned_view(rows, width, c0, pitch, dtype, gpu):
	"""rows: list of 1-D bit arrays (row j's elements, len <= width).  -> (A, buffer): A = buffer[1 : 1 + R, c0 : c0 + width] on the GPU, a
	poisoned margin row above and below, poison in every element that is not a row's."""
	assert c0 >= 1 and c0 + width + 1 <= pitch and width >= 2 * VEC[dtype]
	R = len(rows)
	pat = np.array([0x7F800000, 0x7FC00000, 0x7F61B1E6], dtype=np.uint32)     # +inf, NaN, 3e38
	if dtype == BF16:
		pat = (pat >> 16).astype(np.uint16)
	buf = pat[np.arange((R + 2) * pitch) % 3].reshape(R + 2, pitch)
	for j, r in enumerate(rows):
		assert r.dtype == _bits_dtype(dtype) and r.size <= width
		buf[1 + j, c0:c0 + r.size] = r
	t = torch.from_numpy(buf.view(np.int32 if dtype == F32 else np.int16)).to(gpu).view(dtype)
	assert t.data_ptr() % 16 == 0 or not t.is_cuda
	return t[1:1 + R, c0:c0 + width], t


def _heads(A):
	"""Elements in front of the first 16-byte boundary, per row."""
	es = A.element_size()
	return [((16 - (A.data_ptr() + j * A.stride(0) * es) % 16) % 16) // es for j in range(A.shape[0])]


def _layout(dtype, width, misaligned):
	"""(c0, pitch): aligned = base and pitch multiples of 16 bytes; misaligned = column offset 1 and a pitch that is odd in elements, so
	the head runs through 0 .. VEC - 1 down the rows."""
	v = VEC[dtype]
	if not misaligned:
		return 2 * v, -(-(width + 4 * v) // v) * v
	pitch = width + v + 2
	return 1, pitch + (1 - pitch % 2)


def _reference(rows, lengths, k, dtype):
	want_v = np.full((len(rows), k), NEG_INF32, dtype=np.float32)
	want_i = np.full((len(rows), k), -1, dtype=np.int32)
	for j, (r, n) in enumerate(zip(rows, lengths)):
		want_v[j], want_i[j] = tn.topk_ref(_to_f32(r[:n], dtype), k)
	return want_v, want_i


def _assert_same(got, want_v, want_i, what):
	gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy()
	assert gv.dtype == np.float32 and gi.dtype == np.int32 and gv.shape == want_v.shape and gi.shape == want_i.shape
	bad = np.flatnonzero((gv.view(np.uint32) != want_v.view(np.uint32)).any(axis=1) | (gi != want_i).any(axis=1))
	if bad.size:
		j = int(bad[0])
		c = int(np.flatnonzero((gv[j].view(np.uint32) != want_v[j].view(np.uint32)) | (gi[j] != want_i[j]))[0])
		short = int((gi[j] == -1).sum() - (want_i[j] == -1).sum())
		raise AssertionError(f"{what}: {bad.size} of {gv.shape[0]} rows differ (rows {bad[:10].tolist()}); row {j} first at position {c}: "
							 f"got ({gv[j, c]!r}, {gi[j, c]}), want ({want_v[j, c]!r}, {want_i[j, c]}); {short} more (-inf, -1) entries than wanted")


def _distinct(rng, n, dtype):
	"""n distinct shuffled values: fp32 mixed-sign integers (one +0.0), bf16 distinct patterns."""
	if dtype == F32:
		return _to_bits((rng.permutation(n) - n // 2).astype(np.float32), dtype)
	return tn.distinct_bf16_patterns(rng, n).copy()


def _alphabet(rng, n, dtype):
	"""Five values, {-2 .. 2} / 4: ties everywhere."""
	return _to_bits((rng.integers(-2, 3, n) / 4).astype(np.float32), dtype)


def _const(x, n, dtype):
	return _to_bits(np.full(n, x, dtype=np.float32), dtype)


def _nan_bits(dtype, sign_set=False):
	b = tn.NAN_NEG32 if sign_set else tn.NAN_POS32
	return np.uint32(b) if dtype == F32 else np.uint16(b >> 16)


# ================================================================== A. ragged rows
def _ragged_lengths(dtype, k):
	v = VEC[dtype]
	i_max = 1538 * v + 3
	L = [0, 1, v - 1, v, v + 1, k - 1, k, k + 1]
	L += [64 * v + d for d in (-1, 0, 1)]                                   # one wave step
	for b in (512, 1024, 1536):                                             # seed threshold; first and second turn of the clamp-free loop
		L += [b * v + d for d in range(-v, v + 1)]
	L += [i_max, i_max + 1000, -5]                                          # the last two are clamped
	if dtype == F32:
		L = L + L                                                           # (41 lengths: twice, each meets two different heads)
	L = [L[i] for i in np.random.default_rng(k).permutation(len(L))]        # the four rows of a workgroup get unrelated lengths
	return i_max, L


def _ragged_rows(data, rng, eff, k, dtype):
	rows = []
	for j, n in enumerate(eff):
		if data == "distinct":
			r = _distinct(rng, n, dtype)
		elif data == "ties":
			r = _alphabet(rng, n, dtype)
		else:
			kind = j % 4
			if kind == 0:
				r = _const((1.5, -3.0, 0.0, 7.0)[(j // 4) % 4], n, dtype)
			elif kind == 1:
				r = _const(-np.inf, n, dtype)
			elif kind == 2:
				r = np.full(n, _nan_bits(dtype), dtype=_bits_dtype(dtype))    # an all-NaN prefix: everything padded
			else:                                                             # k - 1 numbers among NaNs: one short of k
				r = np.full(n, _nan_bits(dtype, j % 8 == 7), dtype=_bits_dtype(dtype))
				keep = rng.choice(n, size=min(n, k - 1), replace=False)
				r[keep] = _alphabet(rng, keep.size, dtype)
		rows.append(r)
	return rows


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_rows(ops, gpu, dtype, k, misaligned):
	i_max, lengths = _ragged_lengths(dtype, k)
	eff = [min(max(n, 0), i_max) for n in lengths]
	c0, pitch = _layout(dtype, i_max, misaligned)
	rl = torch.tensor(lengths, dtype=torch.int32, device=gpu)
	for data in ("distinct", "ties", "special"):
		rng = np.random.default_rng([k, VEC[dtype], int(misaligned), len(data)])
		rows = _ragged_rows(data, rng, eff, k, dtype)
		A, _buf = _poisoned_view(rows, i_max, c0, pitch, dtype, gpu)
		assert A.shape == (len(rows), i_max) and A.stride(0) == pitch
		heads = _heads(A)
		assert set(heads) == (set(range(VEC[dtype])) if misaligned else {0})
		got = ops.rowwise_topk_ragged(A, rl, k)
		want_v, want_i = _reference(rows, eff, k, dtype)
		_assert_same(got, want_v, want_i, f"ragged {data}")
		# the fixed-length entry on every prefix that can hold k: bit for bit the same row
		js = [j for j, n in enumerate(eff) if n >= k]
		one = [ops.rowwise_topk(A[j:j + 1, :eff[j]], k) for j in js]
		sel = torch.tensor(js, device=gpu)
		assert torch.equal(torch.cat([o.values for o in one]).view(torch.int32), got.values[sel].view(torch.int32)), f"{data}: values differ from rowwise_topk"
		assert torch.equal(torch.cat([o.indices for o in one]), got.indices[sel]), f"{data}: indices differ from rowwise_topk"


def test_ragged_refusals(ops, gpu):
	from anncur_amd import _lib
	A, _buf = _poisoned_view([_const(1.0, 300, F32)] * 5, 300, 8, 320, F32, gpu)
	rl = torch.full((5,), 300, dtype=torch.int32, device=gpu)
	assert ops.rowwise_topk_ragged(A, rl, 128).indices.shape == (5, 128)
	with pytest.raises(_lib.AnncurHipError):
		ops.rowwise_topk_ragged(A, rl, 129)                                 # above the wave-per-row scan
	with pytest.raises(ValueError):
		ops.rowwise_topk_ragged(A, rl.long(), 10)                           # row_len of the wrong dtype
	with pytest.raises(ValueError):
		ops.rowwise_topk_ragged(A, rl[:4], 10)                              # row_len of the wrong length
	with pytest.raises(ValueError):
		ops.rowwise_topk_ragged(A, torch.cat([rl, rl]), 10)


# ================================================================== B. all-NaN vectors in the seed region
@pytest.mark.parametrize("sign_set", [False, True], ids=["nan7fc0", "nanffc0"])
@pytest.mark.parametrize("k", tn.NAN_BLOCK_KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_vectors_in_the_seed_region(ops, gpu, dtype, k, sign_set):
	"""Rows of tn.nan_block_row (distinct shuffled data, the row's maximum inside the seed region, m in {1, k - 1, k, 200} whole vectors of
	NaN among the first 512) through rowwise_topk, rowwise_topk_ragged and rowwise_topk_gather; every row holds at least k numbers, so every
	output row must be full.

	On the parent's library (measured on an MI355X): the three f32-nan7fc0 cases fail and nothing else in this file does.  In each of them
	the row with m = k - 1 comes back with ONE real entry and k - 1 times (-inf, -1) -- at every length, aligned and misaligned, through
	rowwise_topk, rowwise_topk_gather and rowwise_topk_ragged alike, and no other row differs.  That is exactly what
	tests/test_cpu_topk_reference.py derives for these rows: the device's fmaxf does return the NaN when both operands are NaN.  bf16 rows
	and sign-set NaNs pass on the parent too (bf16 keys NaN patterns 0; a sign-set NaN keys below every number)."""
	v = VEC[dtype]
	nan32 = tn.NAN_NEG32 if sign_set else tn.NAN_POS32
	failures = []                                                           # every entry and layout is run; the report names all that differ

	def check(got, want_v, want_i, what):
		try:
			_assert_same(got, want_v, want_i, what)
		except AssertionError as e:
			failures.append(str(e))
	for misaligned in (False, True):
		all_rows, all_len = [], []
		for length in tn.NAN_BLOCK_LENGTHS:
			rows = [tn.nan_block_row(v, length, k, m, nan32, misaligned) for m in tn.nan_block_ms(k)]
			all_rows += rows
			all_len += [length] * len(rows)
			want_v, want_i = _reference(rows, [length] * len(rows), k, dtype)
			assert (want_i >= 0).all()
			c0, pitch = _layout(dtype, length, misaligned)
			A, _buf = _poisoned_view(rows, length, c0, pitch, dtype, gpu)
			what = f"length {length}, {'mis' if misaligned else ''}aligned, m = {tn.nan_block_ms(k)}"
			check(ops.rowwise_topk(A, k), want_v, want_i, "rowwise_topk, " + what)
			if not misaligned:                                              # (the gather form takes 16-byte aligned rows only)
				cols = sorted({0, 7, 1000, 2047, length - 2, length - 1})
				tables = ops.gather_tables(torch.tensor(cols, dtype=torch.int32, device=gpu), length, dtype)
				got, cq = ops.rowwise_topk_gather(A, k, tables)
				check(got, want_v, want_i, "rowwise_topk_gather, " + what)
				bits = np.stack(rows)[:, cols]
				got_bits = cq.view(torch.int32 if dtype == F32 else torch.int16).cpu().numpy().view(bits.dtype)
				np.testing.assert_array_equal(got_bits, bits)
		# all rows of this layout in one ragged launch
		width = max(all_len)
		c0, pitch = _layout(dtype, width, misaligned)
		A, _buf = _poisoned_view(all_rows, width, c0, pitch, dtype, gpu)
		want_v, want_i = _reference(all_rows, all_len, k, dtype)
		got = ops.rowwise_topk_ragged(A, torch.tensor(all_len, dtype=torch.int32, device=gpu), k)
		check(got, want_v, want_i, f"rowwise_topk_ragged, {'mis' if misaligned else ''}aligned")
	assert not failures, "\n".join(failures)


# ================================================================== C. the workgroup scan, k = 129 .. 2048
SCAN_SIZES = (0, 1, 2051, 8191, 8192, 8193, 10245, 20000)       # 0, 1 stand for k, k + 1
SCAN_OFFSET_SIZES = (8192, 10245)


def _sorted_values(rng, n, dtype, shift):
	"""n ascending distinct values."""
	if dtype == F32:
		return _to_bits((np.arange(n) - n // 2 + shift).astype(np.float32), dtype)
	p = tn.distinct_bf16_patterns(rng, n)
	return p[np.argsort(tn.bf16_bits_to_f32(p), kind="stable")].copy()


def _scan_rows(rng, n, k, dtype):
	"""Seven kinds of row, three of each (row 7 j + i is of kind i)."""
	rows = []
	bt = _bits_dtype(dtype)
	for j in range(3):
		rows.append(_distinct(rng, n, dtype))
		rows.append(_alphabet(rng, n, dtype))
		rows.append(_const((0.25, -1.0, 3.0)[j], n, dtype))                 # the indices must be 0 .. k - 1
		asc = _sorted_values(rng, n, dtype, 7 * j)
		rows.append(asc)                                                    # ascending: every check compacts
		rows.append(asc[::-1].copy())
		r = _const(-np.inf, n, dtype)                                       # mostly -inf, fewer than k finite: -inf by the smallest index
		keep = rng.choice(n, size=min(n, k // 2 + j), replace=False)
		r[keep] = _distinct(rng, keep.size, dtype)
		rows.append(r)
		r = np.full(n, _nan_bits(dtype, j == 2), dtype=bt)                  # fewer than k numbers: padding
		keep = rng.choice(n, size=k - 1 - 40 * j, replace=False)
		r[keep] = _alphabet(rng, keep.size, dtype)
		rows.append(r)
	return rows


TAIL_TIES_AT = 6200


def _tail_threshold_row(rng, n, k, head, dtype):
	"""The row's tail (the elements behind its last whole 16-byte vector: the largest indices, offered before the stream) holds 1.0; k - tail
	elements of 2.0 lie in front of the first compaction, which therefore makes a TAIL element the k-th kept key; eight more 1.0 follow at
	6200 ..: same score as the threshold, smaller index -- they must displace the tail's, which only the composite-key compare can see."""
	tail = (n - head) % VEC[dtype]
	x = np.zeros(n, dtype=np.float32)
	x[rng.choice(2000 if k <= 512 else 4000, size=k - tail, replace=False)] = 2.0
	x[n - tail:] = 1.0
	x[TAIL_TIES_AT:TAIL_TIES_AT + 8] = 1.0
	return _to_bits(x, dtype), tail


@pytest.mark.parametrize("k", [129, 512, 513, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_workgroup_scan(ops, gpu, dtype, k):
	v = VEC[dtype]
	sizes = sorted({k + s if s < 2 else s for s in SCAN_SIZES if s < 2 or s >= k})
	cases = [(n, 0) for n in sizes] + [(n, off) for n in SCAN_OFFSET_SIZES for off in (1, v - 1)]
	failures = []
	for n, off in cases:
		rng = np.random.default_rng([k, v, n, off])
		rows = _scan_rows(rng, n, k, dtype)
		tails = []
		if off == 0:
			c0, pitch = _layout(dtype, n, False)
		else:
			c0 = 2 * v + off
			pitch = n + 5 * v + 1
			pitch += 1 - pitch % 2                                          # odd: the head differs from row to row
			for j in range(len(rows), len(rows) + 2 * v):                   # one row per head, twice
				head = (-((1 + j) * pitch + c0)) % v                        # (the buffer starts on a 16-byte boundary)
				r, tail = _tail_threshold_row(rng, n, k, head, dtype)
				rows.append(r)
				tails.append((j, head, tail))
		A, _buf = _poisoned_view(rows, n, c0, pitch, dtype, gpu)
		want_v, want_i = _reference(rows, [n] * len(rows), k, dtype)
		if off:
			heads = _heads(A)
			assert len(set(heads)) == v and all(heads[j] == head for j, head, _ in tails)
			assert sum(tail > 0 for _, _, tail in tails) >= 2 * (v - 1)
			for j, _, tail in tails:                                        # the later ties are in, the tail's are out
				assert (want_i[j, k - tail:] == TAIL_TIES_AT + np.arange(tail)).all() and (want_v[j, :k - tail] == 2).all()
		assert (want_i[2] == np.arange(k)).all() and (want_i[6] == -1).any() and (want_v[5] == NEG_INF32).any() and (want_i[5] >= 0).all()
		try:
			_assert_same(ops.rowwise_topk(A, k), want_v, want_i, f"I = {n}, column offset {off}")
		except AssertionError as e:
			failures.append(str(e))
	assert not failures, "\n".join(failures)


# ================================================================== D. re-rank
RERANK_CASES = [(kr, ko) for kr in (1, 255, 256, 257, 2048) for ko in (1, 128, 129, 512, 513, 2048) if ko <= kr]


@pytest.mark.parametrize("k_retvr, k_out", RERANK_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rerank(ops, gpu, dtype, k_retvr, k_out):
	"""Tie-heavy integer quarters; distinct candidate ids with -1 holes and ids >= I (they point at poison inside the buffer), in an id tensor
	five columns wider than k_retvr whose extra columns name the one item that would win every row."""
	Q, n, best = 3, 3001, 17
	rng = np.random.default_rng([k_retvr, k_out, VEC[dtype]])
	vals = (rng.integers(-8, 9, (Q, n)) / 4).astype(np.float32)
	vals[:, best] = 100.0
	rows = [_to_bits(vals[j], dtype) for j in range(Q)]
	A, _buf = _poisoned_view(rows, n, VEC[dtype] + 1, n + 3 * VEC[dtype] + 1, dtype, gpu)
	ids = np.full((Q, k_retvr + 5), best, dtype=np.int32)
	others = np.delete(np.arange(n), best)
	for j in range(Q):
		ids[j, :k_retvr] = rng.choice(others, size=k_retvr, replace=False)
		if k_retvr == 1:
			if j: ids[j, 0] = (-1, n)[j - 1]                                 # row 0 keeps its candidate, rows 1 and 2 have none
		else:
			holes = rng.choice(k_retvr, size=max(3, k_retvr // 16), replace=False)
			ids[j, holes] = np.resize(np.array([-1, n, n + 1], dtype=np.int32), holes.size)
	got = ops.rerank(A, torch.from_numpy(ids).to(gpu), k_retvr, k_out)
	want_v = np.empty((Q, k_out), dtype=np.float32)
	want_i = np.empty((Q, k_out), dtype=np.int32)
	for j in range(Q):
		want_v[j], want_i[j] = tn.rerank_ref(vals[j], ids[j, :k_retvr], k_out)
	if k_out == k_retvr:
		assert (want_i == -1).any()                                         # fewer valid ids than k_out: padding
	_assert_same(got, want_v, want_i, "rerank")


# ================================================================== E. denormals and zeros
def _denormal_rows(rng, n, dtype):
	rows = []
	for _ in range(3):
		if dtype == F32:     # distinct denormal patterns of both signs
			mant = rng.choice(np.arange(1, 1 << 23, dtype=np.uint32), size=n, replace=False)
			rows.append((mant | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).astype(np.uint32))
		else:                # bf16 has 254 of them: drawn with replacement, so equal patterns also tie by index
			rows.append((rng.integers(1, 128, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16))
	return rows


@pytest.mark.parametrize("k", [64, 513])
@pytest.mark.parametrize("dtype", DTYPES)
def test_denormals_keep_their_order(ops, gpu, dtype, k):
	for n in (1000, 2100, 5000):                                            # k = 64: the short-row kernel, the wave scan with and without full blocks
		for misaligned in (False, True):
			rng = np.random.default_rng([k, n, VEC[dtype], int(misaligned)])
			rows = _denormal_rows(rng, n, dtype)
			want_v, want_i = _reference(rows, [n] * 3, k, dtype)
			for j, r in enumerate(rows):                                    # (the integer order of the keys: no float compare on this host either)
				key = tn.f32_sortable(_to_f32(r, dtype)).astype(np.int64)
				assert (want_i[j] == np.lexsort((np.arange(n), -key))[:k]).all()
			c0, pitch = _layout(dtype, n, misaligned)
			A, _buf = _poisoned_view(rows, n, c0, pitch, dtype, gpu)
			_assert_same(ops.rowwise_topk(A, k), want_v, want_i, f"denormals, I = {n}, {'mis' if misaligned else ''}aligned")


@pytest.mark.parametrize("k", [64, 513])
@pytest.mark.parametrize("dtype", DTYPES)
def test_zeros_of_both_signs_around_the_kth_place(ops, gpu, dtype, k):
	"""k - 10 positive numbers, 40 zeros of mixed sign, negative numbers: ten zeros belong to the top-k.  The sortable key ranks -0.0 below
	+0.0, the in-order stream's float compare does not, so WHICH ten is left open; asserted is what holds on every path."""
	bt = _bits_dtype(dtype)
	for n in (2100, 5000):
		for misaligned in (False, True):
			rng = np.random.default_rng([k, n, VEC[dtype], int(misaligned), 5])
			rows = []
			for _ in range(3):
				if dtype == F32:
					pos = _to_bits(np.arange(1, k - 9, dtype=np.float32), dtype)
					neg = _to_bits(-np.arange(1, n - k - 29, dtype=np.float32), dtype)
				else:
					nz = tn.FINITE_BF16[1:]
					pos = rng.choice(nz[nz < 0x8000], size=k - 10, replace=False)
					neg = rng.choice(nz[nz >= 0x8000], size=n - k - 30, replace=False)
				zeros = (rng.integers(0, 2, 40).astype(bt) << bt(8 * bt().itemsize - 1)).astype(bt)
				zeros[:2] = [0, 1 << (8 * bt().itemsize - 1)]                # both signs are there
				rows.append(rng.permutation(np.concatenate([pos, zeros, neg]).astype(bt)))
			c0, pitch = _layout(dtype, n, misaligned)
			A, _buf = _poisoned_view(rows, n, c0, pitch, dtype, gpu)
			got = ops.rowwise_topk(A, k)
			gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy()
			for j, r in enumerate(rows):
				x = _to_f32(r, dtype)
				want_v, _ = tn.topk_ref(x, k)
				assert np.array_equal(gv[j], want_v)                         # numerically: 0.0 == -0.0
				assert np.unique(gi[j]).size == k and gi[j].min() >= 0 and gi[j].max() < n
				assert (x[gi[j]].view(np.uint32) == gv[j].view(np.uint32)).all()       # each index points at the very element returned
				assert np.isin(np.flatnonzero(x > want_v[-1]), gi[j]).all() and want_v[-1] == 0
				assert (gi[j, :k - 10] == tn.topk_ref(x, k)[1][:k - 10]).all()       # above the zeros the order is fully defined
