"""The host reference of the GEMM contract (oracle/gemm_chain.py) under test itself: no GPU needed.

tests/test_gpu_gemm_exact.py compares the kernels bit for bit with chain(); this file holds that chain() IS the k-ordered fp32 fmaf
chain (fp64 exactness precondition, equality with the same loop in np.longdouble) and that the grid data separates it from the
results a differently ordered or differently rounded GEMM would give (explicit minimum shares of differing elements), so the GPU
comparison cannot go vacuous.  It also holds the coverage of the case lists the GPU tests run.

The minimum shares are set below what the construction gives at these seeds (11-bit mantissas, K = 19 .. 257: 44 .. 93 % of the
elements differ from the once-rounded product, the reversed chain and a two-way split-K; 8-bit mantissas at K = 100: 11 .. 18 %):
they say "a large part of the block" / "a solid share", not a measured figure.  Run with -s to see the figures."""
import numpy as np
import pytest

from oracle import gemm_chain as G

np_longdouble_is_wider = np.finfo(np.longdouble).nmant >= 63   # x87 extended: 64-bit significand, enough for 24 + 22 bits


def _data(M, N, K, mant_a, mant_b, seed):
	rng = np.random.default_rng(seed)
	return G.grid(rng, (M, K), mant_a), G.grid(rng, (K, N), mant_b)


def _share(x, y):
	return float((x.view(np.int32) != y.view(np.int32)).mean())


@pytest.mark.parametrize("mant", [G.MANT_F32, G.MANT_BF16])
def test_grid_values_are_exact_in_their_formats(mant):
	import torch
	x = G.grid(np.random.default_rng(5), (64, 300), mant)
	s = x.astype(np.float64) * (1 << G.MAX_E)
	assert (s == np.rint(s)).all() and (np.abs(s) < 2.0 ** (mant + G.MAX_E)).all()
	assert len(np.unique(np.abs(x))) > 2 ** mant and (x < 0).any() and (x > 0).any()       # a real spread, both signs
	frac = np.abs(x.astype(np.float64)) % 1.0
	assert all((frac * 2 ** e % 1.0 != 0).any() for e in range(1, G.MAX_E))            # every exponent of the grid is in use
	if mant == G.MANT_BF16:
		t = torch.from_numpy(x)
		assert torch.equal(t.bfloat16().float(), t)


@pytest.mark.parametrize("M,N,K,mant_a,mant_b,seed", [(48, 40, 19, 11, 11, 0), (33, 65, 100, 11, 11, 1), (20, 24, 257, 11, 11, 2), (16, 16, 300, 11, 11, 3),
													   (40, 48, 100, 8, 8, 4), (40, 48, 100, 8, 11, 5), (1, 1, 1, 11, 11, 6), (5, 3, 0, 11, 11, 7)])
def test_fp64_steps_are_exact_and_chain_equals_longdouble_loop(M, N, K, mant_a, mant_b, seed):
	A, B = _data(M, N, K, mant_a, mant_b, seed)
	assert G.assert_exact_in_fp64(A, B)
	# the precondition, restated step by step: every unrounded fp64 step is an integer multiple of 1 / SCALE below 2^52 / SCALE
	acc = np.zeros((M, N), dtype=np.float32)
	for k in range(K):
		step = A[:, k:k + 1].astype(np.float64) * B[k:k + 1, :].astype(np.float64) + acc.astype(np.float64)
		s = step * G.SCALE
		assert (s == np.rint(s)).all() and (np.abs(s) < 2.0 ** 52).all()
		acc = step.astype(np.float32)
	c = G.chain(A, B)
	assert c.dtype == np.float32 and c.shape == (M, N) and np.array_equal(c.view(np.int32), acc.view(np.int32))
	assert np_longdouble_is_wider
	assert np.array_equal(G.chain(A, B, dtype=np.longdouble).view(np.int32), c.view(np.int32))   # no double rounding
	if K == 0:
		assert not c.view(np.int32).any()   # +0.0 everywhere


def test_precondition_refuses_data_off_the_grid():
	A, B = _data(8, 8, 16, 11, 11, 0)
	for bad in (np.float32(2.0 ** -5), np.float32(2.0 ** 11), np.float32(np.nan), np.float32(np.inf)):
		A2 = A.copy()
		A2[3, 5] = bad
		with pytest.raises(AssertionError):
			G.assert_exact_in_fp64(A2, B)
		with pytest.raises(AssertionError):
			G.assert_exact_in_fp64(A, B, cin=np.full((8, 8), bad, dtype=np.float32))


@pytest.mark.parametrize("K,mant,min_share", [(19, 11, 0.35), (33, 11, 0.35), (100, 11, 0.35), (257, 11, 0.35), (100, 8, 0.05)])
def test_chain_differs_from_other_orders_and_roundings(K, mant, min_share):
	"""The test's power: a GEMM that sums in another order, or rounds once at the end, differs from the chain in at least `min_share`
	of the elements of a grid-data product -- far more than the one element a bit-exact comparison needs."""
	A, B = _data(96, 80, K, mant, mant, seed=1000 + K)
	G.assert_exact_in_fp64(A, B)
	c = G.chain(A, B)
	shares = {"once_rounded": _share(c, G.once_rounded(A, B)), "reversed": _share(c, G.chain_reversed(A, B)), "split2": _share(c, G.chain_split2(A, B))}
	print(f"K={K} mant={mant}: share of elements differing from the chain: {shares}")
	for name, s in shares.items():
		assert s >= min_share, (name, s)
	# order inside a k-tile of 16 reversed (the tiles themselves ascending), and the two k of one MFMA swapped
	in_tile = [k for k0 in range(0, K, 16) for k in range(min(K, k0 + 16) - 1, k0 - 1, -1)]
	pair = [k ^ 1 if (k ^ 1) < K else k for k in range(K)]
	assert sorted(in_tile) == list(range(K)) and sorted(pair) == list(range(K))
	more = {"reversed_in_k_tile": _share(c, G.chain(A, B, ks=in_tile)), "swapped_in_mfma_pair": _share(c, G.chain(A, B, ks=pair))}
	print(f"K={K} mant={mant}: {more}")
	assert more["reversed_in_k_tile"] >= min_share and more["swapped_in_mfma_pair"] >= min_share / 5


def test_epilogue_is_exact_for_powers_of_two_and_independent_of_contraction():
	A, B = _data(33, 40, 33, 11, 11, 9)
	cin = G.grid(np.random.default_rng(10), (33, 40))
	G.assert_exact_in_fp64(A, B, cin)
	c = G.chain(A, B)
	for alpha in (-1.0, 0.5, 2.0):
		for beta in (2.0, -0.25):
			want = G.epilogue(c, alpha, beta, cin)
			# mul, mul, add in fp32 with a rounding after each, against the fused form: the same bits, both scalings being exact
			sep = (np.float32(alpha) * c + np.float32(beta) * cin).astype(np.float32)
			wide = (np.longdouble(alpha) * c.astype(np.longdouble) + np.longdouble(beta) * cin.astype(np.longdouble)).astype(np.float32)
			assert np.array_equal(want.view(np.int32), sep.view(np.int32)) and np.array_equal(want.view(np.int32), wide.view(np.int32))
			# alpha applied AFTER the cin term is another result
			late = (alpha * (c.astype(np.float64) + beta * cin.astype(np.float64))).astype(np.float32)
			assert _share(want, late) > 0.9
	assert np.array_equal(G.epilogue(c).view(np.int32), c.view(np.int32))


def test_case_lists_cover_what_they_claim():
	f32 = G.f32_cases()
	assert 24 <= len(f32) <= 48
	assert {c[0] for c in f32} == set(G.F32_MN) and {c[1] for c in f32} == set(G.F32_MN) and {c[2] for c in f32} == set(G.F32_K)
	assert {(c[3], c[4]) for c in f32} == {(l, d) for l in G.LAYOUTS for d in G.DTYPES}
	assert any(c[2] > 32 and c[2] % 16 for c in f32)                                # two k-tiles of 16 plus a tail
	assert any(c[0] > 128 and c[1] > 128 for c in f32)                              # more than one workgroup both ways
	for side in (0, 1):   # each operand: both loaders and the general path, in both dtypes
		assert {(c[3][side], c[4][side]) for c in f32} == {(l, d) for l in "ntpg" for d in (False, True)}
	f64 = G.f64_cases()
	assert 24 <= len(f64) <= 48
	assert {c[0] for c in f64} == set(G.F64_MN) and {c[1] for c in f64} == set(G.F64_MN) and {c[2] for c in f64} == set(G.F64_K)
	assert {c[3] for c in f64} == set(G.LAYOUTS)
	assert any(c[2] > 64 and c[2] % 32 for c in f64) and any(c[0] > 64 and c[1] > 64 for c in f64)
