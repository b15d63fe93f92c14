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


def grid(rng, shape, mant_bits=MANT_F32):
	"""float32 array of fixed-point grid values m * 2^-e, |m| < 2^mant_bits, e in 0 .. MAX_E."""
	m = rng.integers(-(1 << mant_bits) + 1, 1 << mant_bits, size=shape)
	e = rng.integers(0, MAX_E + 1, size=shape)
	return (m * np.exp2(-e.astype(np.float64))).astype(np.float32)


def small_ints(rng, shape, bound=8):
	"""float32 array of integers in [-bound, bound]: products and sums of a few hundred of them are exact in fp32 in any order."""
	return rng.integers(-bound, bound + 1, size=shape).astype(np.float32)


def assert_exact_in_fp64(A, B, cin=None):
	"""The precondition of chain(): the operands are finite multiples of 2^-MAX_E, and no sum of |a||b| terms (so no partial sum in any
	order, rounded to fp32 or not) reaches 2^52 / SCALE.  With cin: it lies on the grid as well, and the epilogue's fp64 sum stays exact
	for |alpha|, |beta| <= 8."""
	ops = [np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)] + ([np.asarray(cin, dtype=np.float64)] if cin is not None else [])
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


def chain(A, B, ks=None, dtype=np.float64):
	"""The fp32 fmaf chain over k in `ks` (default 0 .. K-1 ascending) for the whole M x N block, one numpy expression per k.
	dtype: the wide type the unrounded step is computed in (np.float64; np.longdouble for the self-test)."""
	Aw, Bw = np.asarray(A).astype(dtype), np.asarray(B).astype(dtype)
	M, K = Aw.shape
	acc = np.zeros((M, Bw.shape[1]), dtype=np.float32)
	for k in (range(K) if ks is None else ks):
		acc = (Aw[:, k:k + 1] * Bw[k:k + 1, :] + acc.astype(dtype)).astype(np.float32)
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
