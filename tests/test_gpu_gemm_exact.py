"""anncur_gemm / anncur_gemm_ex (csrc/gemm.hip) against their contract, bit for bit: element (m, n) of ops.gemm(A, B) is the k-ordered
fp32 fmaf chain, k ascending from 0 -- the sentence the bf16x3 route's parity claim rests on (ops.gemm / ops.rescore_topk, csrc/split.hip,
DESIGN 4.4).  The reference is oracle/gemm_chain.py: the chain built from fp64 on fixed-point grid data, where every fp64 step is
exact and the rounding to fp32 is the one an fmaf performs; tests/test_cpu_gemm_chain.py holds that construction on the host and
measures that another summation order or a single final rounding changes 44 .. 93 % of the elements (11-bit mantissas) -- a
tolerance test sees none of that.  Every case asserts the exactness precondition on its own data before it launches anything.

No comparison here has a tolerance.  Operands are views into larger buffers filled with NaN (a read past M, N or K turns the output
into NaN, and stays inside the test's own allocation); outputs are views into buffers filled with one fixed NaN bit pattern, and
every word outside the M x N view must still hold it after the call.

Subnormal inputs and intermediates: the grid here never produces them (the smallest non-zero operand is 2^-4, the smallest non-zero
product 2^-8).  tests/test_gpu_subnormal_exact.py runs the same chain on the same grid scaled by powers of two, with subnormal
partial sums and with subnormal operands, in these buffers.

anncur_gemm_f64 (csrc/gemm64.hip) is held to integer data, where fp64 is exact in any order, at its own tile edges (64 x 64 x 32, MFMA
16 x 16 x 4), in the same poisoned buffers.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import gemm_chain as G

pytestmark = pytest.mark.gpu

DEV = "cuda"

_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}
_POISON = {torch.float32: 0x7fc00123, torch.bfloat16: 0x7fc1, torch.float64: 0x7ff8000000000123}   # NaNs with a payload no kernel produces


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


# ------------------------------------------------------------------ views into poisoned buffers
def _buf_shape(kind, R, C):
	return {"n": (R * C + 16,), "t": (R * C + 16,), "p": (R + 2, C + 5), "pt": (C + 2, R + 5), "s2": (R + 2, 2 * C + 3), "g": (2 * R + 1, 3 * C + 2)}[kind]


def _carve(buf, kind, R, C):
	"""The [R x C] view of layout `kind` inside a buffer of _buf_shape(kind, R, C): slicing only, so it applies to the device buffer
	and to its host image alike.  n: rows contiguous; t: a transposed view; p: padded pitch; pt: padded pitch, transposed;
	s2: column stride 2; g: row stride 2 pitches, column stride 3."""
	if kind == "n":
		return buf[8:8 + R * C].view(R, C)
	if kind == "t":
		return buf[8:8 + R * C].view(C, R).t()
	if kind == "p":
		return buf[1:R + 1, 2:C + 2]
	if kind == "pt":
		return buf[1:C + 1, 2:R + 2].t()
	if kind == "s2":
		return buf[1:R + 1, 1:1 + 2 * C:2]
	if kind == "g":
		return buf[1:1 + 2 * R:2, 1:1 + 3 * C:3]
	raise KeyError(kind)


def _place(x, kind, dtype):
	"""numpy [R x C] -> device view of layout `kind` holding x, surrounded by NaN.  The conversion to `dtype` must be exact."""
	R, C = x.shape
	t = torch.from_numpy(np.ascontiguousarray(x))
	assert torch.equal(t.to(dtype).to(t.dtype), t) or bool(torch.isnan(t).any())
	buf = torch.full(_buf_shape(kind, R, C), float("nan"), dtype=dtype, device=DEV)
	v = _carve(buf, kind, R, C)
	v.copy_(t.to(dtype))
	return v


def _poisoned_out(kind, M, N, dtype):
	buf = torch.full(_buf_shape(kind, M, N), _POISON[dtype], dtype=_INT[dtype], device=DEV)
	return buf, _carve(buf.view(dtype), kind, M, N)


def _assert_buffer(buf, kind, want, dtype, what=""):
	"""The whole buffer, bit for bit: `want` (a host tensor of `dtype`) inside the view, the poison pattern in every other word."""
	M, N = want.shape
	exp = torch.full(_buf_shape(kind, M, N), _POISON[dtype], dtype=_INT[dtype])
	_carve(exp, kind, M, N).copy_(want.contiguous().view(_INT[dtype]))
	got = buf.cpu()
	if not np.array_equal(got.numpy(), exp.numpy()):
		inside = _carve(got, kind, M, N) != _carve(exp, kind, M, N)
		n_in, n_all = int(inside.sum()), int((got != exp).sum())
		first = [tuple(int(i) for i in ix) for ix in inside.nonzero()[:5]]
		raise AssertionError(f"{what}: {n_in} of {M * N} elements differ from the expected bits (first at {first}), "
							 f"{n_all - n_in} words outside the view were overwritten")


def _want(acc_f32, out_dtype):
	t = torch.from_numpy(np.ascontiguousarray(acc_f32))
	return t.bfloat16() if out_dtype == torch.bfloat16 else t   # bf16 output: round-to-nearest-even of the fp32 value


def _operands(M, N, K, a16, b16, seed):
	rng = np.random.default_rng(seed)
	A = G.grid(rng, (M, K), G.MANT_BF16 if a16 else G.MANT_F32)
	B = G.grid(rng, (K, N), G.MANT_BF16 if b16 else G.MANT_F32)
	return A, B


def _dt(is16):
	return torch.bfloat16 if is16 else torch.float32


OUT_KINDS = ("p", "pt", "s2")


# ------------------------------------------------------------------ the shape / layout / dtype matrix
@pytest.mark.parametrize("M,N,K,layout,dtypes", G.f32_cases(), ids=lambda v: "".join(v) if isinstance(v, tuple) and isinstance(v[0], str) else
						 ("".join("hf"[not x] for x in v) if isinstance(v, tuple) else str(v)))
def test_gemm_equals_the_k_ordered_fp32_chain(ops, M, N, K, layout, dtypes):
	A, B = _operands(M, N, K, dtypes[0], dtypes[1], seed=M * 100003 + N * 1009 + K)
	G.assert_exact_in_fp64(A, B)
	acc = G.chain(A, B)
	a, b = _place(A, layout[0], _dt(dtypes[0])), _place(B, layout[1], _dt(dtypes[1]))
	assert a.shape == (M, K) and b.shape == (K, N)
	for out_dtype in (torch.float32, torch.bfloat16):
		for kind in OUT_KINDS:
			buf, out = _poisoned_out(kind, M, N, out_dtype)
			assert ops.gemm(a, b, out=out) is out
			_assert_buffer(buf, kind, _want(acc, out_dtype), out_dtype, f"out {kind} {out_dtype}")
	# a fresh result tensor, both output types
	assert np.array_equal(ops.gemm(a, b).cpu().numpy().view(np.int32), acc.view(np.int32))
	got16 = ops.gemm(a, b, out_dtype=torch.bfloat16).cpu()
	assert np.array_equal(got16.view(torch.int16).numpy(), _want(acc, torch.bfloat16).view(torch.int16).numpy())


@pytest.mark.parametrize("dtypes", G.DTYPES, ids=lambda v: "".join("hf"[not x] for x in v))
@pytest.mark.parametrize("layout", [("n", "n"), ("n", "t"), ("t", "n"), ("t", "t"), ("p", "p"), ("g", "g"), ("pt", "g"), ("g", "pt")], ids="".join)
def test_gemm_chain_every_layout_with_every_dtype_pair(ops, layout, dtypes):
	"""The full cross of layouts and operand types at one ragged two-workgroup shape with two k-tiles and a tail."""
	M, N, K = 129, 65, 33
	A, B = _operands(M, N, K, dtypes[0], dtypes[1], seed=77)
	G.assert_exact_in_fp64(A, B)
	acc = G.chain(A, B)
	a, b = _place(A, layout[0], _dt(dtypes[0])), _place(B, layout[1], _dt(dtypes[1]))
	buf, out = _poisoned_out("p", M, N, torch.float32)
	ops.gemm(a, b, out=out)
	_assert_buffer(buf, "p", _want(acc, torch.float32), torch.float32)
	buf, out = _poisoned_out("s2", M, N, torch.bfloat16)
	ops.gemm(a, b, out=out)
	_assert_buffer(buf, "s2", _want(acc, torch.bfloat16), torch.bfloat16)


# ------------------------------------------------------------------ alpha, beta, cin
@pytest.mark.parametrize("cin_kind", ["separate", "strided", "is_out"])
@pytest.mark.parametrize("beta", [2.0, -0.25])
@pytest.mark.parametrize("alpha", [-1.0, 0.5, 2.0])
def test_gemm_ex_powers_of_two_on_chain_data(ops, alpha, beta, cin_kind):
	"""out = alpha * chain + beta * cin, one rounding: with powers of two both scalings are exact, so the expected bits do not depend on
	whether the epilogue is contracted into an fma.  (-1, 2) is the Newton-Schulz update of the pseudo-inverse."""
	M, N, K = 65, 129, 33
	rng = np.random.default_rng(int((alpha + 2) * 8) * 31 + int((beta + 2) * 8))
	A, B, Cin = G.grid(rng, (M, K)), G.grid(rng, (K, N), G.MANT_BF16), G.grid(rng, (M, N))
	G.assert_exact_in_fp64(A, B, Cin)
	want = G.epilogue(G.chain(A, B), alpha, beta, Cin)
	a, b = _place(A, "p", torch.float32), _place(B, "t", torch.bfloat16)
	if cin_kind == "is_out":
		for kind in OUT_KINDS:   # the in-place update the API permits: cin aliases out element for element
			buf, out = _poisoned_out(kind, M, N, torch.float32)
			out.copy_(torch.from_numpy(Cin))
			_assert_buffer(buf, kind, torch.from_numpy(Cin), torch.float32, "test setup")
			assert ops.gemm(a, b, out=out, alpha=alpha, beta=beta, cin=out) is out
			_assert_buffer(buf, kind, _want(want, torch.float32), torch.float32, f"cin is out, {kind}")
		return
	cin = _place(Cin, "n" if cin_kind == "separate" else "g", torch.float32)
	cin_bits = cin.clone()
	for out_dtype in (torch.float32, torch.bfloat16):
		for kind in OUT_KINDS:
			buf, out = _poisoned_out(kind, M, N, out_dtype)
			ops.gemm(a, b, out=out, alpha=alpha, beta=beta, cin=cin)
			_assert_buffer(buf, kind, _want(want, out_dtype), out_dtype, f"cin {cin_kind}, out {kind} {out_dtype}")
	assert torch.equal(cin, cin_bits)   # cin is read-only
	# alpha alone (no cin): the scaled chain
	got = ops.gemm(a, b, alpha=alpha).cpu().numpy()
	assert np.array_equal(got.view(np.int32), G.epilogue(G.chain(A, B), alpha).view(np.int32))


@pytest.mark.parametrize("dtypes", G.DTYPES, ids=lambda v: "".join("hf"[not x] for x in v))
@pytest.mark.parametrize("cin_kind", ["separate", "strided", "is_out"])
def test_gemm_ex_other_scalars_on_small_integers(ops, cin_kind, dtypes):
	"""alpha = 3, beta = -5 are no powers of two: small-integer data (|x| <= 8, every sum far below 2^24), where nothing rounds and
	the result is exact in any order and under any contraction."""
	M, N, K = 130, 33, 100
	rng = np.random.default_rng(5)
	A, B, Cin = G.small_ints(rng, (M, K)), G.small_ints(rng, (K, N)), G.small_ints(rng, (M, N))
	assert 3 * K * 64 + 5 * 8 < 2 ** 24
	want = (3 * (A.astype(np.float64) @ B.astype(np.float64)) - 5 * Cin.astype(np.float64))
	assert np.abs(want).max() < 2 ** 24
	want = want.astype(np.float32)
	a, b = _place(A, "t", _dt(dtypes[0])), _place(B, "n", _dt(dtypes[1]))
	buf, out = _poisoned_out("pt", M, N, torch.float32)
	if cin_kind == "is_out":
		out.copy_(torch.from_numpy(Cin))
		cin = out
	else:
		cin = _place(Cin, "n" if cin_kind == "separate" else "g", torch.float32)
	ops.gemm(a, b, out=out, alpha=3.0, beta=-5.0, cin=cin)
	_assert_buffer(buf, "pt", torch.from_numpy(want), torch.float32)


# ------------------------------------------------------------------ empty dimensions
@pytest.mark.parametrize("M,N", [(1, 1), (33, 129), (130, 5)])
def test_gemm_k_zero_writes_exact_zeros_or_beta_cin(ops, M, N):
	a = torch.full((M, 4), float("nan"), device=DEV)[:, :0]
	b = torch.full((4, N), float("nan"), device=DEV)[:0, :]
	assert a.shape == (M, 0) and b.shape == (0, N)
	for out_dtype in (torch.float32, torch.bfloat16):
		for kind in OUT_KINDS:
			buf, out = _poisoned_out(kind, M, N, out_dtype)
			ops.gemm(a, b, out=out)
			_assert_buffer(buf, kind, torch.zeros(M, N, dtype=out_dtype), out_dtype, f"K = 0, out {kind} {out_dtype}")   # +0.0, bit for bit
	# empty tensors of their own (null data pointers)
	e = ops.gemm(torch.empty(M, 0, device=DEV), torch.empty(0, N, device=DEV))
	assert e.shape == (M, N) and not e.cpu().view(torch.int32).any()
	Cin = G.grid(np.random.default_rng(M), (M, N))
	cin = _place(Cin, "g", torch.float32)
	for alpha, beta in ((2.0, -0.25), (-1.0, 2.0)):
		buf, out = _poisoned_out("p", M, N, torch.float32)
		ops.gemm(a, b, out=out, alpha=alpha, beta=beta, cin=cin)
		want = G.epilogue(np.zeros((M, N), dtype=np.float32), alpha, beta, Cin)
		assert np.array_equal(want, np.float32(beta) * Cin)
		_assert_buffer(buf, "p", torch.from_numpy(want), torch.float32, f"K = 0 with cin, alpha {alpha}")


@pytest.mark.parametrize("M,N", [(0, 7), (7, 0), (0, 0)])
def test_gemm_empty_output_touches_nothing(ops, M, N):
	K = 5
	a = torch.full((M + 2, K), float("nan"), device=DEV)[:M]
	b = torch.full((K, N + 2), float("nan"), device=DEV)[:, :N]
	buf = torch.full((9, 9), _POISON[torch.float32], dtype=torch.int32, device=DEV)
	out = buf.view(torch.float32)[1:1 + M, 1:1 + N]
	assert ops.gemm(a, b, out=out) is out
	assert ops.gemm(a, b, out=out, alpha=2.0, beta=2.0, cin=out) is out
	assert ops.gemm(a, b).shape == (M, N)
	assert bool((buf.cpu() == _POISON[torch.float32]).all())


# ------------------------------------------------------------------ NaN propagation
@pytest.mark.parametrize("layout", [("n", "n"), ("t", "t"), ("g", "g")], ids="".join)
@pytest.mark.parametrize("M,N,K,m,n,k", [(65, 129, 33, 64, 128, 32), (129, 33, 17, 31, 0, 16), (33, 65, 100, 0, 40, 0)])
def test_one_nan_poisons_exactly_its_row_or_column(ops, M, N, K, m, n, k, layout):
	A, B = _operands(M, N, K, False, False, seed=M + N + K)
	G.assert_exact_in_fp64(A, B)
	acc = G.chain(A, B)
	An, Bn = A.copy(), B.copy()
	An[m, k] = np.nan
	Bn[k, n] = np.nan
	a, b = _place(A, layout[0], torch.float32), _place(B, layout[1], torch.float32)
	got = ops.gemm(_place(An, layout[0], torch.float32), b).cpu().numpy()
	assert np.isnan(got[m]).all() and np.array_equal(np.isnan(got).any(axis=1), np.arange(M) == m)
	assert np.array_equal(np.delete(got, m, axis=0).view(np.int32), np.delete(acc, m, axis=0).view(np.int32))
	got = ops.gemm(a, _place(Bn, layout[1], torch.float32)).cpu().numpy()
	assert np.isnan(got[:, n]).all() and np.array_equal(np.isnan(got).any(axis=0), np.arange(N) == n)
	assert np.array_equal(np.delete(got, n, axis=1).view(np.int32), np.delete(acc, n, axis=1).view(np.int32))


# ------------------------------------------------------------------ launch chunking in ops.gemm
def test_gemm_more_rows_than_one_launch_takes(ops):
	"""M = 65535 * 128 + 5: ops.gemm splits the rows over two launches (grid.y limit); the second one computes the last five rows.
	Small-integer data, compared with the host product in full; with and without cin."""
	M, K, N = 65535 * 128 + 5, 2, 1
	g = torch.Generator(device=DEV).manual_seed(3)
	a = torch.randint(-8, 9, (M, K), generator=g, device=DEV).float()
	cin = torch.randint(-8, 9, (M, N), generator=g, device=DEV).float()
	B = np.array([[3.0], [-7.0]], dtype=np.float32)
	b = _place(B, "n", torch.float32)
	A, Cin = a.cpu().numpy(), cin.cpu().numpy()
	assert A.min() == -8 and A.max() == 8 and len(np.unique(A[-5:])) > 1   # the data reaches the last chunk with something to say
	prod = A.astype(np.float64) @ B.astype(np.float64)
	got = ops.gemm(a, b)
	assert got.shape == (M, N) and np.array_equal(got.cpu().numpy(), prod.astype(np.float32))
	del got
	want = (3 * prod - 5 * Cin.astype(np.float64)).astype(np.float32)
	out = torch.full((M, N), float("nan"), device=DEV)
	ops.gemm(a, b, out=out, alpha=3.0, beta=-5.0, cin=cin)
	assert np.array_equal(out.cpu().numpy(), want)
	assert np.array_equal(cin.cpu().numpy(), Cin)


# ------------------------------------------------------------------ the fp64 GEMM: exact on integers at its own edges
def _f64_operands(M, N, K, seed):
	"""A: random integers in [-9, 9]; B[i][j] = (i * N + j) % 23 - 7 depends on its two indices differently (a transposed fragment or
	C/D map would show).  Every sum is an integer far below 2^53: exact in fp64 in any order."""
	A = np.random.default_rng(seed).integers(-9, 10, size=(M, K)).astype(np.float64)
	B = (np.arange(K * N).reshape(K, N) % 23 - 7).astype(np.float64)
	return A, B


def _int_product(A, B):
	want = A.astype(np.int64) @ B.astype(np.int64)
	assert (np.abs(A).astype(np.int64) @ np.abs(B).astype(np.int64)).max(initial=0) < 2 ** 53
	return want.astype(np.float64)


@pytest.mark.parametrize("M,N,K,layout", G.f64_cases(), ids=lambda v: "".join(v) if isinstance(v, tuple) else str(v))
def test_gemm_f64_exact_on_integers_at_every_edge(ops, M, N, K, layout):
	A, B = _f64_operands(M, N, K, seed=M * 1009 + N * 31 + K)
	want = _int_product(A, B)
	a, b = _place(A, layout[0], torch.float64), _place(B, layout[1], torch.float64)
	for kind in OUT_KINDS:
		buf, out = _poisoned_out(kind, M, N, torch.float64)
		assert ops.gemm_f64(a, b, out=out) is out
		_assert_buffer(buf, kind, torch.from_numpy(want), torch.float64, f"out {kind}")
	assert np.array_equal(ops.gemm_f64(a, b).cpu().numpy().view(np.int64), want.view(np.int64))
	# alpha, beta, cin: a tensor of its own (general strides), then the in-place update
	Cin = np.random.default_rng(K).integers(-5, 6, size=(M, N)).astype(np.float64)
	for alpha, beta in ((3.0, -5.0), (-1.0, 2.0)):
		want2 = (alpha * want + beta * Cin)
		cin = _place(Cin, "g", torch.float64)
		buf, out = _poisoned_out("p", M, N, torch.float64)
		ops.gemm_f64(a, b, out=out, alpha=alpha, beta=beta, cin=cin)
		_assert_buffer(buf, "p", torch.from_numpy(want2), torch.float64, f"cin separate, alpha {alpha}")
		assert np.array_equal(cin.cpu().numpy(), Cin)
		buf, out = _poisoned_out("pt", M, N, torch.float64)
		out.copy_(torch.from_numpy(Cin))
		ops.gemm_f64(a, b, out=out, alpha=alpha, beta=beta, cin=out)
		_assert_buffer(buf, "pt", torch.from_numpy(want2), torch.float64, f"cin is out, alpha {alpha}")


@pytest.mark.parametrize("layout", [("n", "n"), ("t", "t"), ("g", "g")], ids="".join)
@pytest.mark.parametrize("M,N,K", [(65, 33, 77), (17, 130, 33)])
def test_gemm_f64_large_integers_need_every_fp64_bit(ops, M, N, K, layout):
	"""A up to 2^26, B up to 2^20, K <= 77: every sum stays below 2^53, so the result is exact in fp64 -- and wrong as soon as one
	step of the path (a load, a product, the accumulator, the epilogue) is carried out in fp32."""
	rng = np.random.default_rng(M + K)
	A = rng.integers(-(1 << 26), (1 << 26) + 1, size=(M, K)).astype(np.float64)
	B = rng.integers(-(1 << 20), (1 << 20) + 1, size=(K, N)).astype(np.float64)
	want = _int_product(A, B)
	assert (want != want.astype(np.float32).astype(np.float64)).mean() > 0.9   # the data does what the case is about
	a, b = _place(A, layout[0], torch.float64), _place(B, layout[1], torch.float64)
	buf, out = _poisoned_out("s2", M, N, torch.float64)
	ops.gemm_f64(a, b, out=out)
	_assert_buffer(buf, "s2", torch.from_numpy(want), torch.float64)
	Cin = rng.integers(-(1 << 40), 1 << 40, size=(M, N)).astype(np.float64)
	want2 = want - 2 * Cin
	assert np.abs(want2).max() < 2 ** 53
	buf, out = _poisoned_out("p", M, N, torch.float64)
	out.copy_(torch.from_numpy(Cin))
	ops.gemm_f64(a, b, out=out, alpha=1.0, beta=-2.0, cin=out)
	_assert_buffer(buf, "p", torch.from_numpy(want2), torch.float64)


@pytest.mark.parametrize("M,N", [(0, 7), (7, 0)])
def test_gemm_f64_empty_output_touches_nothing(ops, M, N):
	a = torch.full((M + 2, 5), float("nan"), dtype=torch.float64, device=DEV)[:M]
	b = torch.full((5, N + 2), float("nan"), dtype=torch.float64, device=DEV)[:, :N]
	buf = torch.full((9, 9), _POISON[torch.float64], dtype=torch.int64, device=DEV)
	out = buf.view(torch.float64)[1:1 + M, 1:1 + N]
	assert ops.gemm_f64(a, b, out=out) is out
	assert bool((buf.cpu() == _POISON[torch.float64]).all())
