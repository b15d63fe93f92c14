"""The noise contract of the SoftMax item sampling (include/anncur_hip.h) restated in numpy: a helper module of the tests
(tests/test_cpu_sample_host.py, tests/test_gpu_sample_topk.py, tests/test_gpu_adaptive_softmax.py), no test itself.

    mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (uint64, wrapping)
    base = mix64(seed + 0x9E3779B97F4A7C15 * (stream + 1))
    z    = mix64(base ^ (row_key << 32 | item))
    u    = ((z >> 41) + 0.5) * 2^-23
    g    = -log(-log(u))
    key  = float32(float32(s * inv_T) + g)
"""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
	"""splitmix64's finaliser on a Python int or a uint64 array (wrapping)."""
	if isinstance(z, np.ndarray):
		z = z.astype(np.uint64)
		with np.errstate(over="ignore"):
			z = z ^ (z >> np.uint64(30))
			z = z * np.uint64(0xBF58476D1CE4E5B9)
			z = z ^ (z >> np.uint64(27))
			z = z * np.uint64(0x94D049BB133111EB)
			return z ^ (z >> np.uint64(31))
	z &= M64
	z ^= z >> 30
	z = (z * 0xBF58476D1CE4E5B9) & M64
	z ^= z >> 27
	z = (z * 0x94D049BB133111EB) & M64
	return z ^ (z >> 31)


def base(seed, stream):
	return mix64((seed + 0x9E3779B97F4A7C15 * (stream + 1)) & M64)


def counter(seed, stream, row_keys, items):
	"""z of every (row key, item) pair: uint64 [len(row_keys) x len(items)]."""
	rk = (np.asarray(row_keys).astype(np.int64) & 0xffffffff).astype(np.uint64).reshape(-1, 1)
	it = np.asarray(items).astype(np.uint64).reshape(1, -1)
	return mix64(np.uint64(base(seed, stream)) ^ ((rk << np.uint64(32)) | it))


def bits23(seed, stream, row_keys, items):
	"""z >> 41: the 23 bits the uniform is made of, int64 [rows x items]."""
	return (counter(seed, stream, row_keys, items) >> np.uint64(41)).astype(np.int64)


def uniform(seed, stream, row_keys, items):
	"""u as float64 (exact: 24 significant bits)."""
	return (bits23(seed, stream, row_keys, items).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel64(seed, stream, row_keys, items):
	"""g in float64."""
	return -np.log(-np.log(uniform(seed, stream, row_keys, items)))


def bits_from_gumbel(g):
	"""The 23-bit integer u 2^23 - 0.5 recovered from a (device) g, as float64: u = exp(-exp(-g))."""
	return np.exp(-np.exp(-np.asarray(g, dtype=np.float64))) * 2.0 ** 23 - 0.5


def keys32(S, inv_T, G):
	"""key = float32(float32(S * inv_T) + G) from fp32 scores and fp32 noise: two separately rounded fp32 operations."""
	S, G = np.asarray(S, dtype=np.float32), np.asarray(G, dtype=np.float32)
	with np.errstate(invalid="ignore", over="ignore"):
		return (S * np.float32(inv_T)).astype(np.float32) + G


def sample_reference(S, inv_T, G, k, excluded=None):
	"""The sampler's contract on the host: per row the k allowed, non-NaN items with the largest keys, key descending, ties by the smaller id
	(a stable argsort of the negated keys), padded with (-inf, -1).  excluded: per-row collections of ids (or None).  -> (keys f32, ids int32)."""
	key = keys32(S, inv_T, G)
	Q, I = key.shape
	out_v, out_i = np.full((Q, k), -np.inf, dtype=np.float32), np.full((Q, k), -1, dtype=np.int32)
	for q in range(Q):
		allowed = ~np.isnan(key[q])
		if excluded is not None and len(excluded[q]):
			allowed[np.asarray(list(excluded[q]), dtype=np.int64)] = False
		ids = np.nonzero(allowed)[0]
		order = ids[np.argsort(-key[q][ids].astype(np.float64), kind="stable")][:k]
		out_v[q, :order.size], out_i[q, :order.size] = key[q][order], order
	return out_v, out_i


def chi2_first_and_pairs(ids, scores, inv_T=1.0):
	"""Pearson chi-square of a Gumbel top-2 draw's rows `ids` [Q x 2] against the sampling-without-replacement law of softmax(scores * inv_T):
	(chi2 of the first item over the n items, n - 1 degrees of freedom; chi2 of the ordered pairs over the n (n - 1) pairs against the
	Plackett-Luce probabilities p_i p_j / (1 - p_i), n (n - 1) - 1 degrees of freedom)."""
	s = np.asarray(scores, dtype=np.float64) * inv_T
	p = np.exp(s - s.max())
	p /= p.sum()
	n, Q = p.size, ids.shape[0]
	first = np.bincount(ids[:, 0], minlength=n).astype(np.float64)
	chi_first = float(((first - Q * p) ** 2 / (Q * p)).sum())
	pairs = np.bincount(ids[:, 0].astype(np.int64) * n + ids[:, 1], minlength=n * n).reshape(n, n).astype(np.float64)
	pl = p[:, None] * p[None, :] / (1.0 - p[:, None])
	off = ~np.eye(n, dtype=bool)
	assert pairs[~off].sum() == 0          # without replacement: no item twice
	chi_pairs = float(((pairs[off] - Q * pl[off]) ** 2 / (Q * pl[off])).sum())
	return chi_first, chi_pairs
