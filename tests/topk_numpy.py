"""The exact row-wise top-k of include/anncur_hip.h (anncur_rowwise_topk and its ragged / gather forms, anncur_rerank) restated in plain numpy:
score descending, equal scores by ascending index, NaN never selected, -inf an ordinary candidate, (-inf, -1) padding.  A helper module, not a
test: tests/test_cpu_topk_reference.py holds it against torch.topk / a stable argsort and hand-worked rows, tests/test_gpu_rowwise_topk_exact.py
holds the kernels of csrc/topk.hip against it, bit for bit.

Also here, shared by both: the bit-pattern helpers (everything goes through integer views, so no host floating-point mode can flush or
canonicalise a value on its way into a test), the rows with whole 16-byte vectors of NaN inside the region the wave scan seeds its threshold
from, and a host emulation of that seed."""
import numpy as np

NAN_POS32, NAN_NEG32 = 0x7FC00000, 0xFFC00000   # the quiet NaN with the sign bit clear / set (x86's 0/0 gives the second)
SEED_VECS = 512                                 # 16-byte vectors the wave scan takes its seed threshold from (8 per lane)


# ------------------------------------------------------------------ bit patterns
def f32_from_bits(bits):
	"""uint32 patterns -> float32 array with exactly those bits."""
	return np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).view(np.float32)


def bf16_bits_to_f32(bits):
	"""uint16 bf16 patterns -> the float32 values they stand for (exact: the pattern in the high half)."""
	return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(x):
	"""float32 values that ARE bf16 values -> their patterns (asserts that nothing is cut off)."""
	u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
	assert not (u & np.uint32(0xFFFF)).any(), "value is not representable in bf16"
	return (u >> np.uint32(16)).astype(np.uint16)


def _finite_bf16_patterns():
	e = np.arange(1, 255, dtype=np.uint32)[:, None] << 7     # normal exponents only: no denormals, no inf / NaN
	m = np.arange(128, dtype=np.uint32)[None, :]
	pos = (e | m).reshape(-1)
	return np.concatenate([np.zeros(1, dtype=np.uint32), pos, pos | 0x8000]).astype(np.uint16)   # +0.0 but not -0.0


FINITE_BF16 = _finite_bf16_patterns()   # 65 025 patterns, all of different value


def distinct_bf16_patterns(rng, n):
	"""n distinct finite bf16 patterns drawn without replacement: no -0.0, no denormals, so all n VALUES differ."""
	assert n <= FINITE_BF16.size
	return rng.choice(FINITE_BF16, size=n, replace=False)


def f32_sortable(x):
	"""The order-preserving uint32 key of csrc/common.hpp for float32 values (by bit pattern: -0.0 below +0.0)."""
	u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
	return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def f32_unsortable(key):
	"""One key -> the float32 scalar it stands for."""
	k = int(key)
	return np.array([k & 0x7FFFFFFF if k & 0x80000000 else ~k & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------ the reference
def topk_ref(prefix, k):
	"""-> (values float32 [k], indices int32 [k]) of one row (float32, or bf16 given as its float32 values)."""
	x = np.asarray(prefix, dtype=np.float32).reshape(-1)
	idx = np.flatnonzero(~np.isnan(x))
	order = np.lexsort((idx, -x[idx].astype(np.float64)))[:k]      # value descending, then index ascending
	val, ids = np.full(k, -np.inf, dtype=np.float32), np.full(k, -1, dtype=np.int32)
	val[:order.size], ids[:order.size] = x[idx[order]], idx[order]
	return val, ids


def rerank_ref(row, cand_ids, k_out):
	"""The k_out best of row[cand_ids] in the same order; ids outside [0, len(row)) are holes."""
	x = np.asarray(row, dtype=np.float32).reshape(-1)
	c = np.asarray(cand_ids, dtype=np.int64).reshape(-1)
	c = c[(c >= 0) & (c < x.size)]
	c = c[~np.isnan(x[c])]
	order = np.lexsort((c, -x[c].astype(np.float64)))[:k_out]
	val, ids = np.full(k_out, -np.inf, dtype=np.float32), np.full(k_out, -1, dtype=np.int32)
	val[:order.size], ids[:order.size] = x[c[order]], c[order]
	return val, ids


# ------------------------------------------------------------------ rows with all-NaN vectors in the seed region
NAN_BLOCK_LENGTHS = (2048, 2051, 2100, 6000)
NAN_BLOCK_KS = (2, 64, 128)


def nan_block_ms(k):
	return sorted({1, k - 1, k, 200})


def nan_block_row(vec, length, k, m, nan32, misaligned):
	"""One row (uint32 patterns for vec = 4, uint16 for vec = 8) of `length` distinct shuffled values with m blocks of NaN inside its first
	512 vectors.  Aligned: m whole vectors of the grid that starts at element 0.  Misaligned: m runs of 2 vec - 1 elements starting at
	multiples of 2 vec -- wherever the 16-byte grid starts (head 0..vec-1), each run covers exactly one whole vector of it and the runs'
	vectors stay inside the first 512.  The values are shuffled except that the largest lies among elements 8..2039.  The same (arguments) give the same row: the CPU and the GPU test see identical data."""
	rng = np.random.default_rng([vec, length, k, m, int(misaligned)])   # (not the NaN pattern: both patterns get the same row otherwise)
	if vec == 4:
		row = (rng.permutation(length) - length // 2).astype(np.float32).view(np.uint32).copy()   # mixed-sign integers, one +0.0
		nan = np.uint32(nan32)
	else:
		row = distinct_bf16_patterns(rng, length).copy()
		nan = np.uint16(nan32 >> 16)
	if misaligned:
		for u in rng.choice(SEED_VECS // 2 - 1, size=m, replace=False):
			row[u * 2 * vec:u * 2 * vec + 2 * vec - 1] = nan
	else:
		for v in rng.choice(SEED_VECS, size=m, replace=False):
			row[v * vec:(v + 1) * vec] = nan
	# the row's largest value is moved into the seed region (whatever the head): a bound taken from k - 1 NaN maxima and the largest real one
	# then admits exactly one element, also in the rows that are longer than the region
	val = f32_from_bits(row) if vec == 4 else bf16_bits_to_f32(row)
	real = np.flatnonzero(~np.isnan(val))
	top = real[np.argmax(val[real])]
	p = rng.choice(real[(real >= 8) & (real < 2040)])
	row[top], row[p] = row[p], row[top]
	return row


def emulate_f32_seed(row_bits, k, head=0):
	"""The threshold rowwise_topk_wave_kernel<float> starts from when the maximum of an all-NaN vector keeps its NaN pattern (fmaxf of two
	NaNs) and goes through f32_sortable unchecked -> (tau, number of non-NaN elements the stream can still admit: those above tau, or all of
	them while there is no threshold)."""
	x = f32_from_bits(row_bits)
	nvec = (x.size - head) // 4
	real = ~np.isnan(x)
	if nvec < SEED_VECS or k > SEED_VECS:
		return -np.inf, int(real.sum())
	g = x[head:head + 4 * SEED_VECS].reshape(SEED_VECS, 4)
	allnan = np.isnan(g).all(axis=1)
	gmax = np.where(allnan, g[:, 0], np.fmax.reduce(np.where(allnan[:, None], 0, g), axis=1))   # fmax skips a NaN next to a number
	keys = np.sort(f32_sortable(gmax))[::-1]
	kth = int(keys[k - 1])
	tau = np.float32(-np.inf)
	if kth > 0x007FFFFF:                          # the key of -inf
		t = f32_unsortable(kth - 1)
		if abs(t) < np.float32(1.17549435e-38):
			t = np.float32(-1.17549435e-38)
		tau = t
	if not tau > -np.inf:                         # -inf, or a NaN threshold: the kernel's "none yet"
		return tau, int(real.sum())
	return tau, int((x[real] > tau).sum())
