"""Host-side operands and references for subnormal operands, products and sums (no tests here; tests/nonfinite_cases.py is the precedent).
Used by tests/test_cpu_subnormal_reference.py and tests/test_gpu_subnormal_exact.py.  Nothing here is ever read back from a device.

Two kinds of data.

1. ORDER-SENSITIVE: the k-ordered fp32 fmaf chain of oracle/gemm_chain.py on its fixed-point grid, the operands scaled by powers of two
   (CHAIN_CASES).  `sums`: A 2^-70, B 2^-76 -- every operand a normal fp32 and a normal bf16, the products near 2^-130, a good part of
   the partial sums and of the outputs subnormal.  `operands`: A 2^-140 (every non-zero A a subnormal fp32; as bf16: m 2^-133 with
   |m| < 128, exactly the bf16 subnormals), B 2^100 -- the result is 2^-40 (2^-33) times the unscaled chain, all of it normal, and
   all zeros for a device that reads subnormal operands as zero.

2. ORDER-FREE: integers times a power of two (IntCase).  Operands ints 2^a and ints 2^b: every product and every partial sum is
   n 2^u, u = a + b, exactly representable (|n| < 2^23), so every summation order, every MFMA shape and every split of K gives the same
   bits.  `all-sub` (u = -149: the score's bit pattern is |n| plus the sign bit), `straddle` (u = -135: |n| < 512 subnormal, above normal,
   side by side in one row and inside one top-k), `sub-in` (subnormal operands, normal scores; all zero if the operands are flushed).

Each reference comes in three forms: IEEE; DAZ (every subnormal operand replaced by a zero of its sign); FTZ (every subnormal partial
sum or result replaced by a zero of its sign).  A kernel must equal the IEEE form; the other two say what a flush would look like,
and the host asserts before every launch that they are far from the IEEE form where the case is about them."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fused_exact_cases as fx  # noqa: E402
from oracle import gemm_chain as G  # noqa: E402

TINY = 2.0 ** -126            # the smallest normal fp32 -- and the smallest normal bf16: the two formats share the exponent field
F32_STEP = 2.0 ** -149        # the spacing of the fp32 subnormals
BF16_STEP = 2.0 ** -133       # the spacing of the bf16 subnormals (7 mantissa bits)

is_subnormal = G.is_subnormal
flush = G.flush


def bits32(x):
	x = np.ascontiguousarray(x)
	assert x.dtype == np.float32
	return x.view(np.uint32)


def is_subnormal_bits32(u):
	"""From the bit pattern of an fp32: exponent field 0, mantissa not 0."""
	u = np.asarray(u, dtype=np.uint32)
	return ((u >> 23) & 0xff == 0) & ((u & 0x7fffff) != 0)


def is_subnormal_bits16(u):
	"""From the bit pattern of a bf16 (int16 / uint16 view): exponent field 0, mantissa not 0."""
	u = np.asarray(u).astype(np.int64) & 0xffff
	return ((u >> 7) & 0xff == 0) & ((u & 0x7f) != 0)


def to_bf16_exact(a):
	"""numpy -> torch bf16 holding exactly the same numbers (asserted; subnormals included)."""
	a = np.ascontiguousarray(a)
	t = torch.from_numpy(a).to(torch.bfloat16)
	assert (t.double().numpy() == a.astype(np.float64)).all(), "not exact in bf16"
	return t


def f32_to_bf16_rne(x):
	"""float32 numpy -> the bf16 bit patterns (uint16) of round-to-nearest-even, written out on the integer bits: inside the subnormal
	range the same rule applies to the same bit positions (a bf16 is the upper half of an fp32).  The reference for bf16 outputs."""
	u = bits32(x).astype(np.uint64)
	assert not np.isnan(x).any()
	return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------ 1. the scaled chain
CHAIN_CASES = {"sums": (2.0 ** -70, 2.0 ** -76), "operands": (2.0 ** -140, 2.0 ** 100)}
CHAIN_SHAPES = ((33, 65, 100), (129, 31, 17))
CHAIN_LAYOUTS = (("n", "n"), ("t", "t"), ("g", "g"))
MIN_SUBNORMAL_SHARE = 0.2     # of the `sums` outputs
MIN_FLUSH_SHARE = 0.5         # of the elements: how far the flushed variant the case is about lies from the IEEE chain


def chain_operands(case, M, N, K, a16, b16, seed):
	"""(A, B, sa, sb): float32 operands of CHAIN_CASES[case] as the device receives them, and the scales that describe them.
	A bf16 operand has 8 mantissa bits; the bf16 A of `operands` is m 2^-133, |m| < 128 (scale 2^-133, no fraction bits)."""
	sa, sb = CHAIN_CASES[case]
	rng = np.random.default_rng([seed, M, N, K, int(a16), int(b16), list(CHAIN_CASES).index(case)])
	if case == "operands" and a16:
		sa = BF16_STEP
		A = (rng.integers(-127, 128, size=(M, K)) * sa).astype(np.float32)
	else:
		A = G.grid(rng, (M, K), G.MANT_BF16 if a16 else G.MANT_F32, scale=sa)
	B = G.grid(rng, (K, N), G.MANT_BF16 if b16 else G.MANT_F32, scale=sb)
	return A, B, sa, sb


def chain_references(A, B, sa, sb):
	"""{"ieee", "daz", "ftz"} -> float32 [M x N], after the exactness precondition."""
	G.assert_exact_in_fp64(A, B, sa=sa, sb=sb)
	return {"ieee": G.chain(A, B, sa=sa, sb=sb), "daz": G.chain(A, B, daz=True), "ftz": G.chain(A, B, ftz=True)}


def share(x, y):
	return float((bits32(x) != bits32(y)).mean())


def assert_chain_case(case, A, B, refs):
	"""What a chain case promises, on the host, before anything is launched."""
	c = refs["ieee"]
	assert np.isfinite(c).all()
	if case == "sums":
		assert not is_subnormal(A).any() and not is_subnormal(B).any() and np.array_equal(bits32(refs["daz"]), bits32(c))
		assert is_subnormal(c).mean() >= MIN_SUBNORMAL_SHARE, is_subnormal(c).mean()
		assert share(c, refs["ftz"]) >= MIN_FLUSH_SHARE, share(c, refs["ftz"])
	else:
		assert is_subnormal(A[A != 0]).all() and (A != 0).mean() > 0.9 and not is_subnormal(B).any()
		assert not is_subnormal(c).any() and np.array_equal(bits32(refs["ftz"]), bits32(c))
		assert not bits32(refs["daz"]).any()                       # +0 everywhere
		assert share(c, refs["daz"]) >= MIN_FLUSH_SHARE, share(c, refs["daz"])


def epilogue_operands(M, N, K, seed):
	"""Order-free data for the epilogue: A = ints 2^-70, B = ints 2^-77 (|int| <= 8), Cin = ints 2^-147 (|int| <= 200): the accumulator is
	n 2^-147 with |n| <= 64 K, a subnormal like Cin, and alpha acc, beta Cin for alpha, beta in {2, -0.25} are multiples of 2^-149: both
	scalings and the sum are exact in fp32, so the expected bits do not depend on whether the compiler contracts the epilogue into an fma
	(inside the subnormal range a scaling by 1/4 is exact only on such data).  -> (A, B, Cin, acc) float32, acc exact."""
	rng = np.random.default_rng([seed, M, N, K])
	a, b, c = rng.integers(-8, 9, (M, K)), rng.integers(-8, 9, (K, N)), rng.integers(-200, 201, (M, N))
	n = a @ b
	assert (np.abs(a) @ np.abs(b) <= 64 * K).all() and 64 * K * 8 + 200 * 8 < 1 << 22     # every |value| / 2^-149 stays below 2^23: subnormal and exact
	f = lambda v, e: (v.astype(np.float64) * 2.0 ** e).astype(np.float32)
	return f(a, -70), f(b, -77), f(c, -147), f(n, -147)


def epilogue_reference(acc, alpha, beta, cin):
	"""out = alpha acc + beta cin in fp64, rounded once -- after asserting that each scaling alone is exact in fp32, which makes the result
	the same whether the device rounds alpha acc, or beta cin, or neither, before the sum."""
	for s, v in ((alpha, acc), (beta, cin)):
		w = s * v.astype(np.float64)
		assert (w.astype(np.float32).astype(np.float64) == w).all(), "a scaling that rounds: the expected bits would depend on contraction"
	return G.epilogue(acc, alpha, beta, cin)


# ------------------------------------------------------------------ 2. integers times a power of two
INT_CASES = ("all-sub", "straddle", "sub-in")
# name -> (exponent of X, exponent of E): bf16 operands.  sub-in: X = ints 2^-133, the bf16 subnormals themselves
INT_EXPONENTS = {"all-sub": (-70, -79), "straddle": (-60, -75), "sub-in": (-133, 110)}
# fp32 operands of sub-in: column c of X carries the exponent -149 + c % 10 (ints 2^-149 .. 2^-140), E = ints 2^126: scores n 2^-23 again
F32_SUB_IN_E = 126


def _int_matmul(a, b):
	"""The product of two small-integer matrices as int64, through the host BLAS in fp64: exact in any order while every sum of |a||b| stays
	below 2^53 (asserted) -- numpy's own integer product is many times slower at the fused shapes."""
	af, bf = a.astype(np.float64), b.astype(np.float64)
	assert float(np.abs(af).sum(1).max(initial=0)) * float(np.abs(bf).max(initial=0)) < 2.0 ** 53
	p = af @ bf
	out = p.astype(np.int64)
	assert (out == p).all()
	return out


class IntCase:
	"""One order-free problem: X [Q x K] = x 2^a, E [K x I] = e 2^b (float64 arrays holding float32- and, unless f32, bf16-exact numbers),
	N = x e (int64, exact), S = N 2^u the IEEE scores (float64, exactly float32 numbers), S_daz / S_ftz the flushed variants.

	x in [-xmax, xmax], e in [-emax, emax].  straddle: the last four columns shift every score of the problem by the same integer, so that
	the boundary |n| = 2^-126 / 2^u = 512 falls inside the top-k of most queries (k given) or into the upper part of the row (k None).
	f32 (sub-in only): the fp32-operand form, per-column exponents -149 .. -140 on the subnormal side."""

	def __init__(self, name, Q, I, K, k=None, seed=0, xmax=2, emax=3, f32=False):
		assert name in INT_CASES and (not f32 or name == "sub-in") and K >= 2
		g = np.random.default_rng([seed, INT_CASES.index(name), Q, I, K, 0 if k is None else k, int(f32)])
		x = g.integers(-xmax, xmax + 1, (Q, K))
		e = g.integers(-emax, emax + 1, (K, I))
		a, b = INT_EXPONENTS[name]
		col_exp = np.zeros(K, dtype=np.int64)
		if name == "straddle":
			# the last four columns carry the shift: x = 1 there, e = up to four integers of magnitude <= 256 (exact in bf16) that add up to it.
			# The boundary is aimed at the median over the queries of the score at rank k / 8, where the scores of a row lie further apart than
			# the queries differ: the best score of most rows is then a normal number and the k-th a subnormal.
			assert K >= 8
			x[:, K - 4:], e[K - 4:, :] = 1, 0
			n0 = _int_matmul(x, e)
			aim = np.median(np.sort(n0, axis=1)[:, -(max(k // 8, 2) if k else I // 8)])
			shift = int(512 - aim)
			assert abs(shift) <= 1024
			for j in range(4):
				part = int(np.clip(shift, -256, 256))
				e[K - 4 + j, :] = part
				shift -= part
		if f32:
			assert xmax <= 8 and K <= 64
			a, b = -149, F32_SUB_IN_E
			col_exp = np.arange(K) % 10
		self.name, self.Q, self.I, self.K, self.k, self.u, self.f32 = name, Q, I, K, k, a + b, f32
		xs = x << col_exp[None, :]                                          # x 2^(col_exp): the integer X in units of 2^a
		self.N = _int_matmul(xs, e)
		assert int(_int_matmul(np.abs(xs), np.abs(e)).max()) < 1 << 23      # every partial sum in any order: |n| < 2^23
		self.X = xs.astype(np.float64) * 2.0 ** a
		self.E = e.astype(np.float64) * 2.0 ** b
		self.S = self.N.astype(np.float64) * 2.0 ** self.u
		for M in (self.X, self.E, self.S):
			assert (M.astype(np.float32).astype(np.float64) == M).all()     # float32 numbers, all of them
		if not f32:
			to_bf16_exact(self.X), to_bf16_exact(self.E)
		self.S_ftz = flush(self.S.astype(np.float32)).astype(np.float64)
		Xz, Ez = flush(self.X.astype(np.float32)).astype(np.float64), flush(self.E.astype(np.float32)).astype(np.float64)
		self.S_daz = Xz @ Ez                                                # integers times 2^u below 2^23: exact in fp64 in any order
		self._promises()

	def values32(self):
		return self.S.astype(np.float32)

	def _promises(self):
		S32, name = self.values32(), self.name
		sub = is_subnormal(S32)
		if name == "all-sub":
			assert (sub | (S32 == 0)).all() and (S32 == 0).any(1).all() and ((S32 < 0) & sub).any(1).all() and ((S32 > 0) & sub).any(1).all()
			# the bit identity: the pattern of n 2^-149 is |n| plus the sign bit
			want = np.abs(self.N).astype(np.uint32) | np.where(self.N < 0, np.uint32(0x80000000), np.uint32(0))
			assert np.array_equal(bits32(S32), want)
			assert not self.S_ftz.any() and np.array_equal(self.S_daz, self.S)
		elif name == "straddle":
			assert np.array_equal(sub, (self.N != 0) & (np.abs(self.N) < 512))
			assert sub.any(1).all() and (sub.any(1) & (~sub & (S32 != 0)).any(1)).mean() >= 0.9     # side by side in (nearly) every row: one shift serves all queries
			if self.k:
				top = -np.sort(-self.N, axis=1)[:, :self.k]
				both = ((top < 512).any(1) & (top >= 512).any(1)).mean()
				assert both >= 0.75, both                                   # ... and inside the top-k of most queries (one shift serves them all)
			assert np.array_equal(self.S_daz, self.S) and (self.S_ftz != self.S).mean() > 0.2
		else:
			Xs = is_subnormal(self.X.astype(np.float32))
			assert Xs[self.X != 0].all() and (self.X != 0).mean() > 0.5 and not is_subnormal(self.E.astype(np.float32)).any()
			assert not sub.any() and np.array_equal(self.S_ftz, self.S) and not self.S_daz.any() and (self.S != 0).mean() > 0.8
			if not self.f32:
				assert is_subnormal_bits16(to_bf16_exact(self.X).view(torch.int16).numpy())[self.X != 0].all()

	def topk(self, k=None, item_ids=None):
		"""THE top-k (fused_exact_cases.reference_topk on the integers: values descending, ties by ascending row) -> (float32 values, int64 ids)."""
		k = self.k if k is None else k
		val, rows = fx.reference_topk(torch.from_numpy(self.N), k)
		v = (val.numpy().astype(np.float64) * 2.0 ** self.u).astype(np.float32)
		ids = rows.numpy()
		return v, (ids if item_ids is None else np.asarray(item_ids, dtype=np.int64)[ids])

	def gmax(self, tiles, group):
		"""The prepass' group maxima of the sampled tiles from the host scores (fused_exact_cases.reference_gmax) -> float32 [Q x groups]."""
		n = fx.reference_gmax(torch.from_numpy(self.N), np.asarray(tiles), group).double().numpy()
		return (n * 2.0 ** self.u).astype(np.float32)


# ------------------------------------------------------------------ 3. sums of squares in the subnormal range
SUMS_INT_E = -70   # E = ints 2^-70, X small ints: S_hat = n 2^-70, A = (n + delta) 2^-70, err^2 = sum delta^2 2^-140, norm^2 = sum a^2 2^-140


class SumsIntCase:
	"""`sums-int`: sparse X (fused_exact_cases.sparse_x: three coefficients from {1, 2} per query), E = ints in [-2, 2] times 2^-70, the exact
	matrix A = (n + delta) 2^-70 with delta in {-1, 0, 1}.  Every square is an integer times 2^-140 -- a subnormal fp32 -- and every sum of
	them m 2^-140 with m < 2^24: exactly representable below and above 2^-126, so atomics in any order give the same bits.  err^2 stays
	subnormal (m <= I < 2^14); norm^2 may cross into the normal range."""

	def __init__(self, Q, I, K, seed=0):
		g = torch.Generator().manual_seed(seed * 7919 + K)
		e = torch.randint(-2, 3, (K, I), generator=g, dtype=torch.int8)
		X, col, coef = fx.sparse_x(Q, K, g)
		n = fx.sparse_scores(e, col, coef).numpy().astype(np.int64)
		rng = np.random.default_rng([seed, Q, I, K])
		delta = rng.integers(-1, 2, (Q, I))
		self.Q, self.I, self.K = Q, I, K
		self.X = X.double().numpy()
		self.E = e.double().numpy() * 2.0 ** SUMS_INT_E
		self.N, self.A_int = n, n + delta
		self.S = n.astype(np.float64) * 2.0 ** SUMS_INT_E
		self.A = self.A_int.astype(np.float64) * 2.0 ** SUMS_INT_E
		self.err_units = (delta * delta).sum(1)
		self.nrm_units = (self.A_int * self.A_int).sum(1)
		self._promises()

	def _promises(self):
		assert 0 < self.err_units.min() and self.err_units.max() < 1 << 14 and self.nrm_units.max() < 1 << 24
		assert np.abs(self.A_int).max() <= 13                                # every single square: at most 169 2^-140, a subnormal
		to_bf16_exact(self.X), to_bf16_exact(self.E), to_bf16_exact(self.A)
		assert is_subnormal(self.err()).all() and (self.nrm() != 0).all()
		sq = (self.A_int.astype(np.float64) ** 2 * 2.0 ** (2 * SUMS_INT_E)).astype(np.float32)
		assert (is_subnormal(sq) | (sq == 0)).all()                          # FTZ: every term a flushed zero, both sums 0

	def err(self):
		return (self.err_units.astype(np.float64) * 2.0 ** (2 * SUMS_INT_E)).astype(np.float32)

	def nrm(self):
		return (self.nrm_units.astype(np.float64) * 2.0 ** (2 * SUMS_INT_E)).astype(np.float32)
