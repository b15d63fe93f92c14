"""The host references of the subnormal tests (tests/subnormal_cases.py, oracle/gemm_chain.py with scales) under test themselves: no GPU needed.

tests/test_gpu_subnormal_exact.py compares kernels bit for bit with these references.  This file holds that the host forming them does not
flush (float32 arithmetic, the cast from float64, torch's bf16 round trip), that the scaled chain IS the k-ordered fp32 fmaf chain inside
the subnormal range (equality with the same loop in np.longdouble), that the data separates the IEEE result from a flushed one and from
other summation orders by explicit minimum shares, that the all-sub bit identity holds, and that every case keeps its own promises.
The minimum shares are the ones the GPU tests assert before they launch (subnormal_cases.MIN_*); run with -s to see the figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_exact_cases as fx  # noqa: E402
import subnormal_cases as sn  # noqa: E402
from oracle import gemm_chain as G  # noqa: E402

np_longdouble_is_wider = np.finfo(np.longdouble).nmant >= 63


# ------------------------------------------------------------------ this host does not flush
def test_host_float32_arithmetic_keeps_subnormals():
	a = np.float32(2.0 ** -100)
	b = np.float32(2.0 ** -40)
	p = np.array([a], dtype=np.float32) * np.array([b], dtype=np.float32)
	assert p.dtype == np.float32 and p.view(np.uint32)[0] == 1 << 9                     # 2^-140: a subnormal product
	s = np.array([2.0 ** -127], dtype=np.float32)
	assert (s + s).view(np.uint32)[0] == 0x00800000 and (s - np.float32(2.0 ** -128)).view(np.uint32)[0] == 1 << 21
	x = np.arange(1, 9, dtype=np.float32) * np.float32(2.0 ** -149)                     # subnormal operands
	assert np.array_equal(x.view(np.uint32), np.arange(1, 9, dtype=np.uint32)) and (x * np.float32(2.0 ** 30) == np.arange(1, 9) * 2.0 ** -119).all()
	t = torch.from_numpy(x)
	assert torch.equal((t * 2.0).view(torch.int32), torch.arange(2, 18, 2, dtype=torch.int32))       # torch on the host as well


def test_cast_from_float64_rounds_to_nearest_even_inside_the_subnormal_range():
	u = 2.0 ** -149
	wide = np.array([0.5 * u, 0.5 * u * (1 + 2.0 ** -30), 1.5 * u, 2.5 * u, 2.5 * u * (1 + 2.0 ** -30), -0.5 * u, -1.5 * u, (2 ** 23 - 0.5) * u, 0.25 * u])
	got = wide.astype(np.float32).view(np.uint32)
	assert got.tolist() == [0, 1, 2, 2, 3, 0x80000000, 0x80000002, 0x00800000, 0]    # ties to even, up into the first normal number, -0 kept
	assert np.array_equal(wide.astype(np.longdouble).astype(np.float32).view(np.uint32), got)


def test_bf16_round_trip_and_rounding_keep_subnormals():
	m = np.arange(-127, 128)
	x = (m * sn.BF16_STEP).astype(np.float32)
	t = sn.to_bf16_exact(x)                                                              # exact: these ARE the bf16 subnormals
	b = t.view(torch.int16).numpy()
	assert np.array_equal(sn.is_subnormal_bits16(b), m != 0) and np.array_equal(b.astype(np.int64) & 0x7f, np.abs(m))
	assert np.array_equal(sn.is_subnormal_bits32(sn.bits32(x)), m != 0) and np.array_equal(sn.is_subnormal(x), m != 0)
	# rounding fp32 subnormals into bf16 subnormals: torch against the rule written on the integer bits
	rng = np.random.default_rng(0)
	y = rng.integers(-(1 << 23) + 1, 1 << 23, 4096).astype(np.float64) * sn.F32_STEP
	y = np.concatenate([y, np.array([0.5, 1.5, 2.5, -0.5, -1.5, 127.5, 0.49, 0.51]) * sn.BF16_STEP]).astype(np.float32)
	want = sn.f32_to_bf16_rne(y)
	got = torch.from_numpy(y).bfloat16().view(torch.int16).numpy().view(np.uint16)
	assert np.array_equal(got, want)
	assert want[-8:].tolist() == [0, 2, 2, 0x8000, 0x8002, 0x0080, 0, 1]
	with pytest.raises(AssertionError):
		sn.to_bf16_exact(np.array([2.0 ** -134], dtype=np.float32))


def test_bit_helpers_and_flush():
	x = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -127, 2.0 ** -126, -2.0 ** -126, 1.0, np.inf], dtype=np.float32)
	assert sn.is_subnormal(x).tolist() == [False, False, True, True, False, False, False, False]
	assert np.array_equal(sn.is_subnormal_bits32(sn.bits32(x)), sn.is_subnormal(x))
	f = sn.flush(x)
	assert f.dtype == np.float32 and sn.bits32(f).tolist() == [0, 0x80000000, 0, 0x80000000, 0x00800000, 0x80800000, 0x3f800000, 0x7f800000]
	assert sn.is_subnormal(np.array([2.0 ** -1030, 2.0 ** -1000])).tolist() == [True, False]     # by the array's own type


# ------------------------------------------------------------------ the scaled chain
_DT = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("dtypes", _DT, ids=lambda v: "".join("hf"[not x] for x in v))
@pytest.mark.parametrize("M,N,K", sn.CHAIN_SHAPES)
@pytest.mark.parametrize("case", list(sn.CHAIN_CASES))
def test_scaled_chain_is_exact_equals_longdouble_and_keeps_its_promises(case, M, N, K, dtypes):
	A, B, sa, sb = sn.chain_operands(case, M, N, K, dtypes[0], dtypes[1], seed=1)
	refs = sn.chain_references(A, B, sa, sb)
	sn.assert_chain_case(case, A, B, refs)
	c = refs["ieee"]
	for X, is16 in ((A, dtypes[0]), (B, dtypes[1])):
		if is16:
			sn.to_bf16_exact(X)
	if case == "operands" and dtypes[0]:
		assert sn.is_subnormal_bits16(sn.to_bf16_exact(A).view(torch.int16).numpy())[A != 0].all()
	# the precondition, restated step by step in units of sa sb / SCALE
	unit = sa * sb / G.SCALE
	acc = np.zeros((M, N), dtype=np.float32)
	for k in range(K):
		step = A[:, k:k + 1].astype(np.float64) * B[k:k + 1, :].astype(np.float64) + acc.astype(np.float64)
		s = step / unit
		assert (s == np.rint(s)).all() and (np.abs(s) < 2.0 ** 52).all()
		acc = step.astype(np.float32)
	assert np.array_equal(sn.bits32(acc), sn.bits32(c))
	# the result is the unscaled chain times sa sb wherever nothing is subnormal -- and is not where the sums are
	plain = G.chain((A.astype(np.float64) / sa).astype(np.float32), (B.astype(np.float64) / sb).astype(np.float32)).astype(np.float64) * (sa * sb)
	if case == "operands":
		assert np.array_equal(sn.bits32(plain.astype(np.float32)), sn.bits32(c))
	print(f"{case} {M}x{N}x{K} {dtypes}: subnormal outputs {sn.is_subnormal(c).mean():.2f}, differ from ftz {sn.share(c, refs['ftz']):.2f}, from daz {sn.share(c, refs['daz']):.2f}, "
		  f"from reversed {sn.share(c, G.chain_reversed(A, B)):.2f}, from once-rounded {sn.share(c, G.once_rounded(A, B)):.2f}")
	assert np_longdouble_is_wider
	assert np.array_equal(sn.bits32(G.chain(A, B, dtype=np.longdouble)), sn.bits32(c))


def test_sums_case_separates_orders_and_roundings_on_the_fp32_grid():
	"""At M, N, K = 33, 65, 100 on the 11-bit grid: the chain differs from the reversed chain and from the once-rounded product on a large
	part of the block, and from 'every partial sum flushed' almost everywhere."""
	A, B, sa, sb = sn.chain_operands("sums", 33, 65, 100, False, False, seed=1)
	refs = sn.chain_references(A, B, sa, sb)
	c = refs["ieee"]
	assert sn.share(c, refs["ftz"]) >= 0.9 and sn.share(c, G.chain_reversed(A, B)) >= 0.5 and sn.share(c, G.once_rounded(A, B)) >= 0.5
	assert sn.is_subnormal(c).mean() >= sn.MIN_SUBNORMAL_SHARE


def test_precondition_with_scales_refuses_data_off_the_scaled_grid():
	A, B, sa, sb = sn.chain_operands("sums", 8, 8, 16, False, False, seed=0)
	assert G.assert_exact_in_fp64(A, B, sa=sa, sb=sb)
	with pytest.raises(AssertionError):
		G.assert_exact_in_fp64(A, B)                                  # the scales left out: nothing is on the unscaled grid
	A2 = A.copy()
	A2[3, 5] = np.float32(sa * 2.0 ** -5)
	with pytest.raises(AssertionError):
		G.assert_exact_in_fp64(A2, B, sa=sa, sb=sb)
	with pytest.raises(AssertionError):
		G.assert_exact_in_fp64(A, B, sa=3.0, sb=sb)                   # not a power of two
	with pytest.raises(AssertionError):
		G.grid(np.random.default_rng(0), (4, 4), scale=2.0 ** -147)   # below 2^(MAX_E - 149) the grid no longer fits


@pytest.mark.parametrize("M,N,K", [(65, 129, 33)])
def test_epilogue_data_is_exact_under_either_contraction(M, N, K):
	A, B, Cin, acc = sn.epilogue_operands(M, N, K, seed=3)
	for X in (A, B):
		sn.to_bf16_exact(X)
		assert not sn.is_subnormal(X).any()
	assert (sn.is_subnormal(acc) | (acc == 0)).all() and (sn.is_subnormal(Cin) | (Cin == 0)).all() and sn.is_subnormal(acc).mean() > 0.9
	assert np.array_equal(sn.bits32((A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)), sn.bits32(acc))
	for alpha in (2.0, -0.25):
		for beta in (2.0, -0.25):
			want = sn.epilogue_reference(acc, alpha, beta, Cin)
			sep = (np.float32(alpha) * acc + np.float32(beta) * Cin).astype(np.float32)     # mul, mul, add with a rounding after each
			assert np.array_equal(sn.bits32(want), sn.bits32(sep)) and sn.is_subnormal(want).mean() > 0.9
			assert sn.share(want, sn.flush(want)) > 0.9
	# on chain data a scaling by -0.25 of a subnormal accumulator does round: the helper refuses it
	A, B, sa, sb = sn.chain_operands("sums", 33, 65, 100, False, False, seed=1)
	c = G.chain(A, B)
	with pytest.raises(AssertionError):
		sn.epilogue_reference(c, -0.25, 2.0, np.zeros_like(c))
	sn.epilogue_reference(c, 2.0, 2.0, c)


# ------------------------------------------------------------------ integers times a power of two
@pytest.mark.parametrize("name", sn.INT_CASES)
@pytest.mark.parametrize("Q,I,K,k", [(130, 8209, 250, 100), (130, 4113, 513, 100), (17, 4101, 57, 100), (64, 4101, 249, 100), (5, 4101, 300, None)])
def test_int_cases_keep_their_promises(name, Q, I, K, k):
	c = sn.IntCase(name, Q, I, K, k)                                   # (the constructor asserts the promises)
	assert c.S.shape == (Q, I) and c.u == sum(sn.INT_EXPONENTS[name])
	S32 = c.values32()
	assert (S32.astype(np.float64) == c.S).all()
	# the product formed in float32 on this host from the float32 operands gives the same bits (nothing here depends on a wide type)
	q = slice(0, 3)
	acc = np.zeros((3, I), dtype=np.float32)
	X32, E32 = c.X.astype(np.float32), c.E.astype(np.float32)
	for kk in range(K):
		acc = acc + X32[q, kk:kk + 1] * E32[kk:kk + 1, :]
	assert np.array_equal(sn.bits32(acc) & 0x7fffffff, sn.bits32(S32[q]) & 0x7fffffff) and (acc == S32[q]).all()
	if k:
		v, ids = c.topk()
		assert v.shape == (Q, k) and (np.diff(v.astype(np.float64), axis=1) <= 0).all()
		assert np.array_equal(v, np.take_along_axis(S32, ids, axis=1))
		tie = v[:, 1:] == v[:, :-1]
		assert tie.mean() > 0.2 and (np.diff(ids, axis=1)[tie] > 0).all()      # tie-heavy rows, ties by ascending row
		perm = np.random.default_rng(1).permutation(I)
		v2, ids2 = c.topk(item_ids=perm)
		assert np.array_equal(v2, v) and np.array_equal(ids2, perm[ids])
		if name == "all-sub":
			assert (sn.is_subnormal(v) | (v == 0)).all()
		if name == "sub-in":
			assert not sn.is_subnormal(v).any() and (v[:, 0] > 0).all()


def test_case_lists_cover_what_they_claim():
	assert set(sn.CHAIN_CASES) == {"sums", "operands"} and set(sn.CHAIN_SHAPES) == {(33, 65, 100), (129, 31, 17)}
	assert set(sn.CHAIN_LAYOUTS) == {("n", "n"), ("t", "t"), ("g", "g")} and set(G.DTYPES) == {(a, b) for a in (False, True) for b in (False, True)}
	sa, sb = sn.CHAIN_CASES["sums"]
	assert sa * sb / G.SCALE < sn.F32_STEP and sa * 2.0 ** -G.MAX_E >= sn.TINY and sb * 2.0 ** -G.MAX_E >= sn.TINY          # products below fp32's last bit, operands normal
	sa, sb = sn.CHAIN_CASES["operands"]
	assert sa * 2.0 ** G.MANT_F32 <= sn.TINY and sa * 2.0 ** -G.MAX_E >= sn.F32_STEP and sa * sb * 2.0 ** -(2 * G.MAX_E) >= sn.TINY   # A subnormal and exact, products normal
	assert any(M > 128 for M, N, K in sn.CHAIN_SHAPES) and any(K > 32 and K % 16 for M, N, K in sn.CHAIN_SHAPES) and any(K % 16 == 1 for M, N, K in sn.CHAIN_SHAPES)
	assert sn.INT_CASES == ("all-sub", "straddle", "sub-in") and [sum(sn.INT_EXPONENTS[n]) for n in sn.INT_CASES] == [-149, -135, -23]
	assert 2.0 ** sn.INT_EXPONENTS["sub-in"][0] == sn.BF16_STEP and 2.0 ** (-149 + sn.F32_SUB_IN_E) == 2.0 ** -23
	# the fused bodies: the seven sweep bodies, k on both sides of the wave-level select's 128, every Kp class
	assert set(fx.BODIES) == {"ladder", "staged", "mfma32", "qt1", "q16", "ring", "wide"}
	assert {k for b in fx.BODIES.values() for k in b[3]} == {100, 700} and {b[0] for b in fx.BODIES.values()} == {64, 128, 256, 512, 640}
	assert {v[0] for b in fx.BODIES.values() for v in b[3].values()} == {8209, 44817, 4113} and all(b[1] <= b[0] for b in fx.BODIES.values())


def test_all_sub_bit_identity():
	c = sn.IntCase("all-sub", 17, 4101, 250)
	b = sn.bits32(c.values32())
	assert np.array_equal(b & 0x7fffffff, np.abs(c.N).astype(np.uint32)) and np.array_equal(b >> 31 != 0, c.N < 0)
	assert int(np.abs(c.N).max()) < 1 << 16        # ... so the coarse threshold's 16-bit key prefix is that of +-0 for every query


def test_sub_in_fp32_form():
	c = sn.IntCase("sub-in", 70, 4101, 56, 10, xmax=8, f32=True)
	X32 = c.X.astype(np.float32)
	assert sn.is_subnormal(X32[c.X != 0]).all() and X32.view(np.uint32).max() & 0x7fffffff < 1 << 13
	exps = {int(np.log2(abs(v) / sn.F32_STEP)) for v in X32[:, :10][c.X[:, :10] != 0]}
	assert min(exps) == 0 and max(exps) >= 9       # 2^-149 .. 2^-140 and a little above (ints up to 8)
	assert not c.S_daz.any() and (c.S != 0).mean() > 0.8


def test_group_maxima_reference_on_scaled_scores():
	c = sn.IntCase("straddle", 9, 8209, 250, 100)
	tiles = np.array([0, 7, 100, 255])
	for group in (4, 16):
		g = c.gmax(tiles, group)
		rows = fx.group_rows(group)
		want = np.stack([c.values32()[:, (t * 32 + rows).reshape(-1)].reshape(9, rows.shape[0], -1).max(2) for t in tiles], axis=1).reshape(9, -1)
		assert np.array_equal(sn.bits32(g), sn.bits32(want))


@pytest.mark.parametrize("K", [56, 120, 250])
def test_sums_int_case(K):
	c = sn.SumsIntCase(130, 4101, K)
	assert np.array_equal(c.X @ (c.E * 2.0 ** -sn.SUMS_INT_E), c.N)
	d = (c.S - c.A) ** 2
	assert (sn.is_subnormal(d.astype(np.float32)) | (d == 0)).all() and (d.astype(np.float32).astype(np.float64) == d).all()
	# summed in float32 on this host, forwards and backwards: the same bits as the integer count
	for order in (slice(None), slice(None, None, -1)):
		e = np.zeros(130, dtype=np.float32)
		n = np.zeros(130, dtype=np.float32)
		for col, col_a in zip(d.astype(np.float32).T[order], (c.A ** 2).astype(np.float32).T[order]):
			e, n = e + col, n + col_a
		assert np.array_equal(sn.bits32(e), sn.bits32(c.err())) and np.array_equal(sn.bits32(n), sn.bits32(c.nrm()))
