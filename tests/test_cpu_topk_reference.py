"""tests/topk_numpy.py (the host statement of the exact top-k the GPU tests compare with) against torch.topk and a stable argsort,
against hand-worked rows, and -- for the rows with all-NaN vectors that tests/test_gpu_rowwise_topk_exact.py feeds the scan -- the
emulation of the fp32 seed threshold: those rows must be able to show a threshold seeded from a NaN maximum.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from topk_numpy import (FINITE_BF16, NAN_BLOCK_KS, NAN_BLOCK_LENGTHS, NAN_NEG32, NAN_POS32, bf16_bits_to_f32, distinct_bf16_patterns,
						emulate_f32_seed, f32_from_bits, f32_sortable, f32_to_bf16_bits, f32_unsortable, nan_block_ms, nan_block_row, rerank_ref,
						topk_ref)  # noqa: E402

INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _same(got, val, idx):
	v, i = got
	assert v.dtype == np.float32 and i.dtype == np.int32
	np.testing.assert_array_equal(v.view(np.uint32), np.asarray(val, dtype=np.float32).view(np.uint32))
	np.testing.assert_array_equal(i, np.asarray(idx, dtype=np.int32))


@pytest.mark.parametrize("n, k", [(1, 1), (37, 37), (1000, 64), (5000, 129), (5000, 2048)])
def test_tie_free_rows_agree_with_torch_topk(n, k):
	g = np.random.default_rng(n + k)
	x = (g.permutation(n) - n // 2).astype(np.float32)
	w = torch.topk(torch.from_numpy(x), k)
	_same(topk_ref(x, k), w.values.numpy(), w.indices.numpy())


@pytest.mark.parametrize("n, k", [(5, 5), (1000, 1), (1000, 64), (5000, 513), (3000, 2048)])
def test_tie_heavy_rows_agree_with_a_stable_argsort(n, k):
	g = np.random.default_rng(n * 7 + k)
	x = (g.integers(-2, 3, n) / 4).astype(np.float32)
	order = np.argsort(-x, kind="stable")[:k]
	_same(topk_ref(x, k), x[order], order)
	tv = torch.topk(torch.from_numpy(x), k).values.numpy()        # (torch leaves the tie ORDER open: values only)
	np.testing.assert_array_equal(topk_ref(x, k)[0], tv)


def test_hand_worked_rows():
	_same(topk_ref([1, NAN, 3, 3, -INF, INF, NAN, 2], 4), [INF, 3, 3, 2], [5, 2, 3, 7])                   # NaN skipped, +inf first, tie by index
	_same(topk_ref([1, NAN, 3, 3, -INF, INF, NAN, 2], 8), [INF, 3, 3, 2, 1, -INF, -INF, -INF], [5, 2, 3, 7, 0, 4, -1, -1])   # -inf a candidate, then padding
	_same(topk_ref([NAN, NAN, NAN], 2), [-INF, -INF], [-1, -1])                                              # all NaN: all padding
	_same(topk_ref([], 3), [-INF] * 3, [-1] * 3)                                                           # an empty prefix
	_same(topk_ref([-INF, -INF, -INF, -INF], 2), [-INF, -INF], [0, 1])                                      # -inf by smallest index
	_same(topk_ref([NAN, 5, NAN], 3), [5, -INF, -INF], [1, -1, -1])                                          # fewer selectable elements than k
	_same(topk_ref([7, 7, 7, 7, 7], 3), [7, 7, 7], [0, 1, 2])
	# both NaN patterns are NaN
	x = f32_from_bits([NAN_POS32, 0x3F800000, NAN_NEG32, 0x40000000])
	_same(topk_ref(x, 3), [2, 1, -INF], [3, 1, -1])


def test_denormals_and_zeros_are_not_flushed_on_this_host():
	"""The reference ranks through float64: a host that flushed fp32 denormals on the way would tie them all.  Held against the integer
	order of the sortable keys."""
	g = np.random.default_rng(3)
	mant = g.choice(np.arange(1, 1 << 23, dtype=np.uint32), size=3000, replace=False)
	bits = mant | (g.integers(0, 2, 3000).astype(np.uint32) << np.uint32(31))
	x = f32_from_bits(bits)
	assert (np.abs(x.astype(np.float64)) > 0).all() and (np.abs(x) < np.float32(1.17549435e-38)).all()
	keys = f32_sortable(x).astype(np.int64)
	order = np.argsort(-keys, kind="stable")[:500]
	_same(topk_ref(x, 500), x[order], order)
	# zeros of either sign are equal: index order
	z = f32_from_bits([0x80000000, 0, 0x80000000, 0x00000001, 0x80000001])
	v, i = topk_ref(z, 5)
	np.testing.assert_array_equal(i, [3, 0, 1, 2, 4])
	np.testing.assert_array_equal(v.view(np.uint32), z.view(np.uint32)[[3, 0, 1, 2, 4]])


def test_bit_pattern_helpers():
	assert FINITE_BF16.size == 65025 and FINITE_BF16.dtype == np.uint16
	v = bf16_bits_to_f32(FINITE_BF16)
	assert np.isfinite(v).all() and np.unique(v).size == v.size                        # distinct VALUES: one zero, no denormals
	assert not (FINITE_BF16 == 0x8000).any()
	assert ((FINITE_BF16 & 0x7F80) != 0).sum() == 65024
	p = distinct_bf16_patterns(np.random.default_rng(0), 20000)
	assert np.unique(p).size == 20000 and np.isin(p, FINITE_BF16).all()
	np.testing.assert_array_equal(f32_to_bf16_bits(bf16_bits_to_f32(p)), p)
	with pytest.raises(AssertionError):
		f32_to_bf16_bits(np.float32(1.0001))
	x = f32_from_bits([0x00000001, 0x80000001, NAN_POS32, NAN_NEG32])
	np.testing.assert_array_equal(x.view(np.uint32), [0x00000001, 0x80000001, NAN_POS32, NAN_NEG32])
	# the sortable key: monotone, -0.0 below +0.0, and its inverse
	s = np.sort(np.random.default_rng(1).standard_normal(1000).astype(np.float32))
	assert (np.diff(f32_sortable(s).astype(np.int64)) >= 0).all()
	assert f32_sortable(f32_from_bits([0x80000000]))[0] + 1 == f32_sortable(f32_from_bits([0]))[0]
	for b in (0x3F800000, 0xBF800000, 0x00000001, 0xFF800000):
		assert f32_unsortable(f32_sortable(f32_from_bits([b]))[0]).view(np.uint32) == b
	assert f32_sortable(f32_from_bits([NAN_POS32]))[0] == 0xFFC00000 and f32_sortable(f32_from_bits([NAN_NEG32]))[0] == 0x003FFFFF


def test_rerank_ref_with_holes():
	row = np.array([5, 1, 5, 3, NAN, 9, 5], dtype=np.float32)
	_same(rerank_ref(row, [6, -1, 2, 7, 3, 100, 0], 3), [5, 5, 5], [0, 2, 6])           # ties by id whatever the candidates' order; -1, 7, 100 are holes
	_same(rerank_ref(row, [6, -1, 2, 7, 3, 100, 0], 6), [5, 5, 5, 3, -INF, -INF], [0, 2, 6, 3, -1, -1])
	_same(rerank_ref(row, [4, -1, 7], 2), [-INF, -INF], [-1, -1])                         # a NaN score is never selected; nothing valid is left
	_same(rerank_ref(row, [5], 1), [9], [5])
	g = np.random.default_rng(2)
	x = (g.integers(-8, 9, 400) / 4).astype(np.float32)
	c = g.choice(400, 300, replace=False)
	masked = np.full(400, NAN, dtype=np.float32)
	masked[c] = x[c]
	_same(rerank_ref(x, c, 50), *topk_ref(masked, 50))                                 # = the top-k of the row with everything else masked


# ------------------------------------------------------------------ the fp32 seed on the GPU test's own rows
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("k", NAN_BLOCK_KS)
def test_nan_block_rows_can_expose_a_seed_taken_from_a_nan_maximum(k, misaligned):
	"""With k - 1 all-NaN vectors of the sign-clear pattern counted as the largest maxima, the bound is the LARGEST real group maximum: the
	stream admits that one element where k are wanted.  With NaNs of the other sign, or with the NaN maxima keyed 0, the bound is valid on
	the same rows.  (m = k and m = 200 make the bound itself NaN, which the kernel reads as "no threshold": those rows pass either way.)"""
	for length in NAN_BLOCK_LENGTHS:
		for head in (range(4) if misaligned else (0,)):
			row = nan_block_row(4, length, k, k - 1, NAN_POS32, misaligned)
			x = f32_from_bits(row)
			if (length - head) // 4 < 512:              # (2048 elements behind a head: 511 vectors, the kernel takes no seed)
				assert emulate_f32_seed(row, k, head)[1] == (~np.isnan(x)).sum() >= k
				continue
			g = np.isnan(x[head:head + 2048].reshape(512, 4)).all(axis=1)
			assert g.sum() == k - 1, "every NaN block must cover exactly one whole vector of the row's grid"
			assert (~np.isnan(x)).sum() >= k
			tau, admitted = emulate_f32_seed(row, k, head)
			assert admitted == 1 < k, (length, head, tau, admitted)
			# the same row with sign-set NaNs: their key is below every number's, the bound holds
			tau, admitted = emulate_f32_seed(nan_block_row(4, length, k, k - 1, NAN_NEG32, misaligned), k, head)
			assert admitted >= k, (length, head, tau, admitted)
		for m in nan_block_ms(k):
			for nan32 in (NAN_POS32, NAN_NEG32):
				for vec in (4, 8):
					row = nan_block_row(vec, length, k, m, nan32, misaligned)
					x = f32_from_bits(row) if vec == 4 else bf16_bits_to_f32(row)
					sel = x[~np.isnan(x)]
					assert sel.size >= k and np.unique(sel).size == sel.size and not (np.signbit(sel) & (sel == 0)).any()
					v, i = topk_ref(x, k)
					assert (i >= 0).all()                       # a full row is wanted: short output is the failure
