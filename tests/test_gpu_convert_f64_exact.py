"""anncur_convert_f64 (ops.convert_f64, convert64_kernel in csrc/gemm64.hip) -- the widening, scaling and rounding helper of the fp64
pseudo-inverse -- bit for bit: f64 -> f32 over every fp32 value's rounding neighbourhood (the value, the tie above it, the tie +- one fp64
ulp) and the overflow / denormal / zero / inf / NaN edges against numpy's astype, bf16 -> f64 over all 65536 patterns, f32 -> f64 over
the same fp32 patterns (exact, denormals included), f64 -> f64 with alpha and a device divisor against numpy's (alpha * x) / d -- one rounded
product, then one rounded division: the kernel's order is the contract -- and every pair on plain / transposed source and destination views
at the shapes around the 256-element launch tail.

No comparison here has a tolerance.  Sources are interior views of NaN-filled buffers, destinations interior views whose surroundings must
keep their NaN.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)   # as in tests/test_gpu_small_kernels_exact.py
E_INVALID = -1
NP = {F32: (np.float32, np.uint32, np.int32, torch.int32), BF16: (None, np.uint16, np.int16, torch.int16), F64: (np.float64, np.uint64, np.int64, torch.int64)}
PAIRS = [(F32, F64), (BF16, F64), (F64, F64), (F64, F32)]
PAIR_IDS = ["f32-f64", "bf16-f64", "f64-f64", "f64-f32"]
MODES = ["plain", "src_t", "dst_t", "both_t"]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


# ------------------------------------------------------------------ bits in, bits out
def _from_bits(bits, dtype):
	"""numpy unsigned patterns [R x C] -> host tensor of `dtype` with exactly those bits."""
	_, u, i, _ = NP[dtype]
	return torch.from_numpy(np.ascontiguousarray(bits, dtype=u).view(i)).view(dtype)


def _bits(t):
	"""tensor -> numpy unsigned patterns."""
	_, u, _, ti = NP[t.dtype]
	return t.contiguous().view(ti).cpu().numpy().view(u)


def _ragged(patterns, n_cols):
	"""1-D array of bit patterns -> [rows x n_cols] with zero patterns filling the last row."""
	rows = -(-patterns.size // n_cols)
	full = np.zeros(rows * n_cols, dtype=patterns.dtype)
	full[:patterns.size] = patterns
	return full.reshape(rows, n_cols)


def _view(M, N, dtype, transposed):
	"""An [M x N] view (row-major, or a transposed one) inside a NaN-filled buffer with a padded pitch -> (view, buffer, mask of the view)."""
	buf = torch.full((N + 5, M + 7) if transposed else (M + 5, N + 7), float("nan"), dtype=dtype, device=DEV)
	inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
	if transposed:
		inside[2:N + 2, 3:M + 3] = True
		return buf[2:N + 2, 3:M + 3].t(), buf, inside
	inside[2:M + 2, 3:N + 3] = True
	return buf[2:M + 2, 3:N + 3], buf, inside


def _run(ops, src_bits, src_dtype, dst_dtype, mode="plain", alpha=1.0, divide_by=None):
	"""convert_f64 of the patterns `src_bits` [M x N] between interior views -> the destination's patterns; the NaN around the destination
	view must survive (the NaN around the source shows up in the result if it is read)."""
	M, N = src_bits.shape
	src, _, _ = _view(M, N, src_dtype, mode in ("src_t", "both_t"))
	dst, dbuf, inside = _view(M, N, dst_dtype, mode in ("dst_t", "both_t"))
	src.copy_(_from_bits(src_bits, src_dtype).to(DEV))
	assert np.array_equal(_bits(src), src_bits)                                   # (the copy into the view kept every bit)
	div = None if divide_by is None else torch.tensor([divide_by], dtype=F64, device=DEV)
	out = ops.convert_f64(src, dst, alpha, divide_by=div)
	assert out.data_ptr() == dst.data_ptr()
	assert bool(torch.isnan(dbuf)[~inside].all()), "an element outside the destination view was written"
	return _bits(dst)


def _same_but_nan(got, want, nan, sign):
	"""Non-NaN results equal bit for bit; where the input is a NaN the result is a NaN of the same sign (payloads are not compared)."""
	assert np.array_equal(got[~nan], want[~nan])
	u, width = got.dtype.type, got.dtype.itemsize * 8
	inf = {32: 0x7f800000, 64: 0x7ff0000000000000}[width]
	g = got[nan]
	assert ((g & u(2 ** (width - 1) - 1)) > u(inf)).all()
	assert np.array_equal(g >> u(width - 1), sign[nan].astype(got.dtype))


def _f32_patterns():
	up = np.arange(65536, dtype=np.uint32)
	return np.concatenate([(up << 16) | lo for lo in LOW_HALVES]).astype(np.uint32)


# ------------------------------------------------------------------ f64 -> f32: every rounding neighbourhood
def _f64_to_f32_inputs():
	pat = _f32_patterns()
	pat = pat[(pat & 0x7fffffff) < 0x7f7fffff]                                    # finite, and with a finite successor
	v = pat.view(np.float32).astype(np.float64)
	vp = (pat + np.uint32(1)).view(np.float32).astype(np.float64)                 # the next fp32 value away from zero
	mid = (v + vp) / 2                                                            # exact: two adjacent 24-bit numbers
	away = np.where(np.signbit(v), -np.inf, np.inf)
	neigh = np.concatenate([v, mid, np.nextafter(mid, away), np.nextafter(mid, -away)])
	fmax, half_ulp = float(np.finfo(np.float32).max), 2.0 ** 103
	edge = [fmax + half_ulp,                                                     # a tie between FLT_MAX and 2^128: to even, i.e. inf
			np.nextafter(fmax + half_ulp, 0.0),                                   # one fp64 ulp below it: FLT_MAX
			2.0 ** 128, fmax,
			0.5 * 2.0 ** -149, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, (2.0 ** 23 - 1.5) * 2.0 ** -149, (2.0 ** 23 - 0.5) * 2.0 ** -149,   # ties between fp32 denormals
			2.0 ** -150, np.nextafter(2.0 ** -150, 1.0),                           # the tie rounds to 0, the next double to 2^-149
			5e-324, 2.0 ** -1060, 2.0 ** -1022,                                   # fp64 denormals and the smallest normal: +-0 with the sign
			0.0, np.inf]
	edge = np.array(edge + [-e for e in edge], dtype=np.float64)
	assert (np.abs(edge[:3]) > fmax).all() and edge[0] - edge[1] == 2.0 ** 75     # (one ulp of a double near 2^128)
	nan = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001, 0x7fffffffffffffff, 0xffffffffffffffff],
				   dtype=np.uint64)
	return np.concatenate([neigh.view(np.uint64), edge.view(np.uint64), nan])


def test_f64_to_f32_over_every_rounding_neighbourhood(ops):
	"""Reference: numpy's astype(float32) of the same doubles."""
	src = _ragged(_f64_to_f32_inputs(), 517)
	x = src.view(np.float64)
	with np.errstate(over="ignore", under="ignore", invalid="ignore"):
		want = x.astype(np.float32).view(np.uint32)
	nan = np.isnan(x)
	got = _run(ops, src, F64, F32)
	_same_but_nan(got, want, nan, src >> np.uint64(63))
	# the data does what the case is about (asserted on the host's reference):
	xs, w = src[~nan], want[~nan]
	frac = xs & np.uint64((1 << 29) - 1)                                          # the 29 bits a normal fp32 result drops
	keep_lsb = (xs >> np.uint64(29)) & np.uint64(1)
	normal = ((w & 0x7f800000) != 0) & ((w & 0x7f800000) != 0x7f800000)
	tie = normal & (frac == np.uint64(1 << 28))
	assert (tie & (keep_lsb == 0)).sum() > 10000 and (tie & (keep_lsb == 1)).sum() > 10000          # ties of both parities
	assert ((w[tie] & 1) == 0).all()                                                                  # ... which all went to even
	exp64 = ((xs >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
	exp32 = ((w >> 23) & 0xff).astype(np.int64) - 127
	assert (normal & (exp32 == exp64 + 1)).sum() > 100                                                # carries into the next exponent
	finite_in = (xs & np.uint64(0x7ff0000000000000)) != np.uint64(0x7ff0000000000000)
	assert (finite_in & ((w & 0x7fffffff) == 0x7f800000)).sum() >= 4                                  # overflow to inf
	assert (((w & 0x7f800000) == 0) & ((w & 0x7fffff) != 0)).sum() > 1000                             # denormal results
	assert (((w & 0x7fffffff) == 0) & ((xs << np.uint64(1)) != 0)).sum() >= 8                         # non-zero inputs that round to +-0
	assert ((w == 0x80000000) & ((xs << np.uint64(1)) != 0)).any()                                    # ... with their sign


# ------------------------------------------------------------------ widening: exact
def test_bf16_to_f64_over_every_pattern(ops):
	src = _ragged(np.arange(65536, dtype=np.uint16), 261)
	f32 = (src.astype(np.uint32) << 16).view(np.float32)
	nan = np.isnan(f32)
	with np.errstate(invalid="ignore"):                                          # (signalling NaN patterns)
		want = f32.astype(np.float64).view(np.uint64)
	got = _run(ops, src, BF16, F64)
	assert nan.sum() == 2 * 127
	_same_but_nan(got, want, nan, src >> np.uint16(15))


def test_f32_to_f64_over_every_upper_half(ops):
	"""Widening is exact, and an fp32 denormal must arrive as the same number (a flush to zero would show)."""
	src = _ragged(_f32_patterns(), 517)
	f32 = src.view(np.float32)
	nan = np.isnan(f32)
	with np.errstate(invalid="ignore"):                                          # (signalling NaN patterns)
		want = f32.astype(np.float64).view(np.uint64)
	den = ((src & 0x7f800000) == 0) & ((src & 0x7fffff) != 0)
	assert nan.sum() == 6 * 2 * 127 + 2 * 5 and den.sum() == 6 * 2 * 128 - 2 and (want[den] << np.uint64(1) != 0).all()   # (this host does not flush them either)
	got = _run(ops, src, F32, F64)
	_same_but_nan(got, want, nan, src >> np.uint32(31))


# ------------------------------------------------------------------ f64 -> f64: alpha and divide_by, the kernel's order
def _generic_doubles(n, seed):
	"""+-(1 + f) 2^e with e across the whole exponent range, the denormals included."""
	g = np.random.default_rng(seed)
	x = np.ldexp(1.0 + g.random(n), g.integers(-1074, 1020, n)) * g.choice([-1.0, 1.0], n)
	return x.astype(np.float64)


ALPHA, DIVISOR = 0.3, 7.1      # neither a power of two: both the product and the division round


def test_f64_scaled_copy_rounds_the_product_then_the_division(ops):
	x = _ragged(_generic_doubles(20000, 5).view(np.uint64), 517).view(np.float64)
	src = x.view(np.uint64)
	with np.errstate(under="ignore"):
		want = ((ALPHA * x) / DIVISOR).view(np.uint64)
		other = ((ALPHA / DIVISOR) * x).view(np.uint64)
	assert (want != other).sum() > 1000                                           # (the documented order differs from the one the header used to give)
	assert np.array_equal(_run(ops, src, F64, F64, alpha=ALPHA, divide_by=DIVISOR), want)
	assert np.array_equal(_run(ops, src, F64, F64), src)                          # alpha = 1, no divisor: a copy
	assert np.array_equal(_run(ops, src, F64, F64, alpha=-2.5), (-2.5 * x).view(np.uint64))


# ------------------------------------------------------------------ strides, launch tails
def _stride_case_bits(M, N, src_dtype, dst_dtype, seed):
	g = np.random.default_rng(seed)
	if src_dtype == F64:
		lim = 120 if dst_dtype == F32 else 1000                                   # f64 -> f32: inside fp32's range after scaling
		x = np.ldexp(1.0 + g.random(M * N), g.integers(-lim, lim, M * N)) * g.choice([-1.0, 1.0], M * N)
		return x.reshape(M, N).view(np.uint64)
	if src_dtype == F32:
		b = g.integers(0, 2 ** 32, M * N, dtype=np.uint64).astype(np.uint32)
		b[(b & 0x7f800000) == 0x7f800000] &= np.uint32(0x807fffff)              # inf / NaN patterns become denormals
		return b.reshape(M, N)
	b = g.integers(0, 2 ** 16, M * N, dtype=np.uint64).astype(np.uint16)
	b[(b & 0x7f80) == 0x7f80] &= np.uint16(0x807f)
	return b.reshape(M, N)


def _as_f64(bits, dtype):
	if dtype == F64:
		return bits.view(np.float64)
	if dtype == F32:
		return bits.view(np.float32).astype(np.float64)
	return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _check_strided(ops, M, N, src_dtype, dst_dtype, mode):
	bits = _stride_case_bits(M, N, src_dtype, dst_dtype, M * 1000 + N)
	x = _as_f64(bits, src_dtype)
	np_dst, u_dst, _, _ = NP[dst_dtype]
	with np.errstate(under="ignore"):
		want_div = ((ALPHA * x) / DIVISOR).astype(np_dst).view(u_dst)
		want_mul = (-2.5 * x).astype(np_dst).view(u_dst)
		want_copy = x.astype(np_dst).view(u_dst)
	assert np.array_equal(_run(ops, bits, src_dtype, dst_dtype, mode, alpha=ALPHA, divide_by=DIVISOR), want_div)
	assert np.array_equal(_run(ops, bits, src_dtype, dst_dtype, mode, alpha=-2.5), want_mul)
	assert np.array_equal(_run(ops, bits, src_dtype, dst_dtype, mode), want_copy)


@pytest.mark.parametrize("M,N", [(1, 1), (1, 255), (1, 256), (1, 257), (17, 15), (255, 3), (64, 300)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src_dtype,dst_dtype", PAIRS, ids=PAIR_IDS)
def test_every_pair_on_strided_views_around_the_launch_tail(ops, src_dtype, dst_dtype, mode, M, N):
	_check_strided(ops, M, N, src_dtype, dst_dtype, mode)


def test_every_pair_at_2048_x_1024(ops):
	"""The largest block pinv.py converts (8192 workgroups), each pair in another of the four view modes."""
	for (src_dtype, dst_dtype), mode in zip(PAIRS, ("both_t", "src_t", "dst_t", "plain")):
		_check_strided(ops, 2048, 1024, src_dtype, dst_dtype, mode)


# ------------------------------------------------------------------ empty, invalid
@pytest.mark.parametrize("M,N", [(0, 5), (5, 0)])
@pytest.mark.parametrize("src_dtype,dst_dtype", PAIRS, ids=PAIR_IDS)
def test_empty_shapes_touch_nothing(ops, src_dtype, dst_dtype, M, N):
	for mode in MODES:
		got = _run(ops, np.zeros((M, N), dtype=NP[src_dtype][1]), src_dtype, dst_dtype, mode, alpha=2.0, divide_by=3.0)   # (_run: every NaN outside survives)
		assert got.shape == (M, N)


@pytest.mark.parametrize("src_dtype,dst_dtype", [(F32, F32), (F64, BF16), (BF16, F32), (F32, BF16), (BF16, BF16)], ids=lambda d: str(d).split(".")[-1])
def test_unsupported_pair_is_invalid_and_writes_nothing(ops, src_dtype, dst_dtype):
	from anncur_amd import _lib
	code = {F32: _lib.F32, BF16: _lib.BF16, F64: _lib.F64}
	lib = _lib.load()
	src = torch.ones((4, 6), dtype=src_dtype, device=DEV)
	dst, dbuf, _ = _view(4, 6, dst_dtype, False)
	rc = lib.anncur_convert_f64(ops._p(src), code[src_dtype], 6, 1, ops._p(dst), code[dst_dtype], dst.stride(0), 1, 4, 6, 1.0, None, ops._stream())
	torch.cuda.synchronize()
	assert rc == E_INVALID and b"unsupported dtype pair" in lib.anncur_last_error()
	assert bool(torch.isnan(dbuf).all())
	# a dtype code that is none of the three, and a negative dimension
	assert lib.anncur_convert_f64(ops._p(src), 7, 6, 1, ops._p(dst), _lib.F64, dst.stride(0), 1, 4, 6, 1.0, None, ops._stream()) == E_INVALID
	assert lib.anncur_convert_f64(ops._p(src), _lib.F32, 6, 1, ops._p(dst), _lib.F64, dst.stride(0), 1, -1, 6, 1.0, None, ops._stream()) == E_INVALID
	torch.cuda.synchronize()
	assert bool(torch.isnan(dbuf).all())
