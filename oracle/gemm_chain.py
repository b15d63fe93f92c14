"""TEST INFRASTRUCTURE ONLY -- host statement of the strided GEMMs' contract, defined without the GPU.

The contract (anncur_amd/ops.py gemm, csrc/split.hip): element (m, n) of gemm(A, B) is the k-ordered fp32 fmaf chain

	acc = 0;  for k = 0 .. K-1:  acc = fmaf(A[m, k], B[k, n], acc)

Python 3.10 has no math.fma, so the chain is built from fp64 on FIXED-POINT GRID DATA: every operand is m * 2^-e with an integer
|m| < 2^11 (|m| < 2^8 where the operand must be bf16-exact) and e in 0..4.  Every product is then an integer multiple of 2^-8 below
2^22, every partial sum (rounded to fp32 or not) an integer multiple of 2^-8 far below 2^52 * 2^-8, so float64(a) * float64(b) +
float64(acc) is computed WITHOUT rounding and acc = float32(that) is the single rounding an fmaf performs.
assert_exact_in_fp64() checks that precondition on the data at hand; tests/test_cpu_gemm_chain.py holds the construction against
the same loop in np.longdouble and measures how strongly it separates the chain from other summation orders.

Also here: the covering sets of (shape, layout, dtype) cases the GPU tests run, so that the CPU test can hold their coverage.
"""
import numpy as np

MANT_F32 = 11    # |m| < 2^11: fp32 operands
MANT_BF16 = 8    # |m| < 2^8: operands that must survive a round trip through bf16
MAX_E = 4        # value = m * 2^-e, e in 0 .. MAX_E
SCALE = float(1 << (2 * MAX_E))   # every product and every sum is an integer multiple of 1 / SCALE


def _pow2(s):
	"""A scale must be a power of two (scaling by it is exact in fp64 wherever the result is representable)."""
	s = float(s)
	assert s > 0 and np.frexp(s)[0] == 0.5, s
	return s


def grid(rng, shape, mant_bits=MANT_F32, scale=1.0):
	"""float32 array of fixed-point grid values m * 2^-e, |m| < 2^mant_bits, e in 0 .. MAX_E, times the power of two `scale`.  The scaled
	values must be float32 numbers (normal or subnormal): scale >= 2^(MAX_E - 149)."""
	m = rng.integers(-(1 << mant_bits) + 1, 1 << mant_bits, size=shape)
	e = rng.integers(0, MAX_E + 1, size=shape)
	wide = m * np.exp2(-e.astype(np.float64)) * _pow2(scale)
	out = wide.astype(np.float32)
	assert (out.astype(np.float64) == wide).all()   # nothing rounded: the grid fits under the scale
	return out


def small_ints(rng, shape, bound=8):
	"""float32 array of integers in [-bound, bound]: products and sums of a few hundred of them are exact in fp32 in any order."""
	return rng.integers(-bound, bound + 1, size=shape).astype(np.float32)


def assert_exact_in_fp64(A, B, cin=None, sa=1.0, sb=1.0):
	"""The precondition of chain(): the operands are finite multiples of 2^-MAX_E, and no sum of |a||b| terms (so no partial sum in any
	order, rounded to fp32 or not) reaches 2^52 / SCALE.  With cin: it lies on the grid as well, and the epilogue's fp64 sum stays exact
	for |alpha|, |beta| <= 8.
	sa, sb: A and B are grid values times these powers of two (cin: times sa * sb).  The scales are taken off first (exact in fp64), so
	the same bounds hold in units of u = sa * sb / SCALE.  A partial sum rounded to fp32 is a multiple of its own ulp, a power of two that
	is either >= u or so small that the sum was representable and did not move: every accumulator stays a multiple of u, inside the
	subnormal range too (ulp 2^-149), and every fp64 step spans fewer than 53 bits.  u itself must be a normal fp64 and the largest sum a
	finite fp32 (asserted)."""
	sa, sb = _pow2(sa), _pow2(sb)
	assert sa * sb / SCALE >= 2.0 ** -960 and sa * sb / SCALE * 2.0 ** 52 < 2.0 ** 127
	ops =[np.asarray(A, dtype=np.float64) / sa, np.asarray(B, dtype=np.float64) / sb] + ([np.asarray(cin, dtype=np.float64) / (sa * sb)] if cin is not None else [])
	for x in ops:
		assert np.isfinite(x).all()
		s = x * (1 << MAX_E)
		assert (s == np.rint(s)).all() and (np.abs(s) < 2.0 ** (MANT_F32 + MAX_E)).all()
	a, b = np.abs(ops[0]) * (1 << MAX_E), np.abs(ops[1]) * (1 << MAX_E)
	total = a @ b if a.shape[1] else np.zeros((a.shape[0], b.shape[1]))   # integers: exact in fp64 whatever order the host BLAS sums in, while below 2^53
	if cin is not None:
		total = 8 * total + 8 * np.abs(ops[2]) * SCALE
	assert (total == np.rint(total)).all() and (total.max() if total.size else 0.0) < 2.0 ** 52
	return True


def is_subnormal(x):
	"""Elementwise: a non-zero float32 / float64 below the smallest normal number of its own type (exponent field 0)."""
	x = np.asarray(x)
	return (x != 0) & (np.abs(x) < np.finfo(x.dtype).tiny)


def flush(x):
	"""Every subnormal replaced by a zero of its sign (what a flush-to-zero mode does to a result, a denormals-are-zero mode to an operand)."""
	x = np.asarray(x)
	return np.where(is_subnormal(x), np.copysign(x.dtype.type(0), x), x)


def chain(A, B, ks=None, dtype=np.float64, sa=1.0, sb=1.0, daz=False, ftz=False):
	"""The fp32 fmaf chain over k in `ks` (default 0 .. K-1 ascending) for the whole M x N block, one numpy expression per k.
	dtype: the wide type the unrounded step is computed in (np.float64; np.longdouble for the self-test).
	sa, sb: A and B are grid values times these powers of two, as grid(scale=) makes them and as the device receives them (float32
	numbers, subnormals included).  Given, the chain checks its own precondition with them.  The step is as exact as on the unscaled
	grid, and its one rounding to fp32 is round-to-nearest-even inside the subnormal range as well.
	daz / ftz: the two ways a flushing device would differ -- every subnormal operand read as a zero of its sign; every subnormal
	partial sum replaced by a zero of its sign."""
	A32, B32 = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
	if sa != 1.0 or sb != 1.0:
		assert_exact_in_fp64(A32, B32, sa=sa, sb=sb)
	if daz:
		A32, B32 = flush(A32), flush(B32)
	Aw, Bw = A32.astype(dtype), B32.astype(dtype)
	M, K = Aw.shape
	acc = np.zeros((M, Bw.shape[1]), dtype=np.float32)
	for k in (range(K) if ks is None else ks):
		acc = (Aw[:, k:k + 1] * Bw[k:k + 1, :] + acc.astype(dtype)).astype(np.float32)
		if ftz:
			acc = flush(acc)
	return acc


def chain_reversed(A, B):
	"""The same chain with k descending."""
	return chain(A, B, ks=range(np.asarray(A).shape[1] - 1, -1, -1))


def chain_split2(A, B):
	"""A two-way split-K: the chains over the lower and the upper half of k, added with one fp32 rounding."""
	K = np.asarray(A).shape[1]
	lo, hi = chain(A, B, ks=range(0, K // 2)), chain(A, B, ks=range(K // 2, K))
	return (lo.astype(np.float64) + hi.astype(np.float64)).astype(np.float32)


def once_rounded(A, B):
	"""The exact product rounded to fp32 once (what an fp64 or a wide-accumulator GEMM would return)."""
	return (np.asarray(A).astype(np.float64) @ np.asarray(B).astype(np.float64)).astype(np.float32)


def epilogue(acc, alpha=1.0, beta=0.0, cin=None, dtype=np.float32):
	"""out = alpha * acc (+ beta * cin) as the kernels' epilogue states it, evaluated in fp64 and rounded once.  With alpha and beta
	powers of two both scalings are exact, so this is the result whether or not the compiler contracts the epilogue into an fma."""
	v = alpha * acc.astype(np.float64)
	if cin is not None:
		v = v + beta * np.asarray(cin).astype(np.float64)
	return v.astype(dtype)


# ------------------------------------------------------------------ covering sets of the GPU tests
# Operand placements (tests/test_gpu_gemm_exact.py carves them out of NaN-filled buffers):
#   n = rows contiguous, t = a transposed view (columns contiguous), p = rows with a padded pitch, g = neither stride 1 (buf[1::2, 1::3])
# For A, n / p make k the unit-stride index (the kfast loader), t does not; for B it is the other way round; g takes the general path.
LAYOUTS = (("n", "n"), ("n", "t"), ("t", "n"), ("t", "t"), ("p", "p"), ("g", "g"))
DTYPES = ((False, False), (True, False), (False, True), (True, True))   # (A is bf16, B is bf16)

# fp32 kernel: tile 128 x 128 x 16, a wave 64 x 64 = 2 x 2 MFMA tiles of 32 x 32
F32_MN = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
F32_K = (1, 2, 15, 16, 17, 31, 33, 100)
# fp64 kernel: tile 64 x 64 x 32, a wave 32 x 32, MFMA 16 x 16 x 4
F64_MN = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
F64_K = (0, 1, 3, 4, 5, 31, 32, 33, 77)


def _covering(mn, ks, rounds):
	"""len(rounds) passes over the M values; pass r pairs M = mn[i] with N = mn[(mul * i + off) % n] (a permutation: n is prime) and
	walks the K values with a pass-dependent offset."""
	n = len(mn)
	out = []
	for r, (mul, off) in enumerate(rounds):
		for i in range(n):
			out.append((mn[i], mn[(mul * i + off) % n], ks[(i + 3 * r) % len(ks)]))
	return out


def f32_cases():
	"""[(M, N, K, (a_layout, b_layout), (a_bf16, b_bf16))]: 33 shapes, every M and N value three times on each side, every K value,
	every (layout pair, dtype pair) combination at least once."""
	shapes = _covering(F32_MN, F32_K, ((1, 0), (3, 4), (7, 9)))
	return [(M, N, K, LAYOUTS[j % 6], DTYPES[(j // 6) % 4]) for j, (M, N, K) in enumerate(shapes)]


def f64_cases():
	"""[(M, N, K, (a_layout, b_layout))]: 33 shapes of the fp64 kernel's matrix, the layouts in turn."""
	shapes = _covering(F64_MN, F64_K, ((1, 0), (3, 4), (7, 9)))
	return [(M, N, K, LAYOUTS[(j + j // 6) % 6]) for j, (M, N, K) in enumerate(shapes)]
