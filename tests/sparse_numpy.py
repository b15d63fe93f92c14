"""The sparse inner-product route of include/anncur_hip.h (csrc/sparse.hip) restated in plain numpy.  A helper module, not a test:
tests/test_cpu_sparse_host.py holds the model to the int64 dense product and shows that the summation order is visible in its data,
tests/test_gpu_sparse_exact.py holds the kernel to it bit for bit.

A CSR matrix is a (indptr int64 [n + 1], indices int32, data float32) triple in canonical form: term ids strictly ascending inside a row."""
import numpy as np


class CSR:
	"""The duck type the library accepts for scipy.sparse.csr_matrix: .indptr / .indices / .data / .shape (and .format)."""
	format = "csr"

	def __init__(self, indptr, indices, data, shape):
		self.indptr, self.indices, self.data, self.shape = indptr, indices, data, tuple(shape)

	@property
	def triple(self):
		return self.indptr, self.indices, self.data


def csr_from_rows(rows, V):
	"""rows: a list of (term ids ascending, values) -> CSR [len(rows) x V]."""
	indptr = np.zeros(len(rows) + 1, dtype=np.int64)
	indptr[1:] = np.cumsum([len(t) for t, _ in rows])
	indices = np.concatenate([np.asarray(t, dtype=np.int32) for t, _ in rows] + [np.zeros(0, dtype=np.int32)])
	data = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows] + [np.zeros(0, dtype=np.float32)])
	return CSR(indptr, indices, data, (len(rows), V))


def densify(m):
	"""CSR -> dense float32 [n x V] (a stored zero becomes an ordinary zero)."""
	out = np.zeros(m.shape, dtype=np.float32)
	for r in range(m.shape[0]):
		a, b = m.indptr[r], m.indptr[r + 1]
		out[r, m.indices[a:b]] = m.data[a:b]
	return out


def postings_ref(m):
	"""The term-major index of a CSR item matrix: (term_ptr int64 [V + 1], post_item int32 [nnz] ascending inside a term, post_val float32)."""
	n, V = m.shape
	rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(m.indptr))
	order = np.argsort(m.indices, kind="stable")
	term_ptr = np.zeros(V + 1, dtype=np.int64)
	term_ptr[1:] = np.cumsum(np.bincount(m.indices, minlength=V))
	return term_ptr, rows[order], m.data[order]


def scores_ref(queries, items, descending=False):
	"""S [Q x n] float32: for every (query, item) the chain over the terms they share, in ascending term order (descending: the reverse, for
	the test that the order matters), from +0.0f, acc = fl(acc + fl(w * v)) with both roundings in float32."""
	term_ptr, post_item, post_val = postings_ref(items)
	Q, n = queries.shape[0], items.shape[0]
	S = np.zeros((Q, n), dtype=np.float32)
	for q in range(Q):
		a, b = queries.indptr[q], queries.indptr[q + 1]
		terms, weights = queries.indices[a:b], queries.data[a:b]
		order = range(len(terms) - 1, -1, -1) if descending else range(len(terms))
		acc = S[q]
		for j in order:
			lo, hi = term_ptr[terms[j]], term_ptr[terms[j] + 1]
			it = post_item[lo:hi]                      # distinct items: the fancy-indexed update below touches each once
			prod = (np.float32(weights[j]) * post_val[lo:hi]).astype(np.float32)
			acc[it] = (acc[it] + prod).astype(np.float32)
	return S


def group_maxima(S):
	"""GM [Q x ceil(n / 64)]: the maximum of every 64 consecutive items (fmax from NaN: a NaN is skipped)."""
	Q, n = S.shape
	G = -(-n // 64)
	pad = np.full((Q, G * 64), np.nan, dtype=np.float32)
	pad[:, :n] = S
	with np.errstate(invalid="ignore"):
		return np.fmax.reduce(pad.reshape(Q, G, 64), axis=2)


def _random_rows(rng, n, V, lo, hi, values):
	rows = []
	for _ in range(n):
		c = int(rng.integers(lo, min(hi, V) + 1))
		t = np.sort(rng.choice(V, size=c, replace=False)).astype(np.int32)
		rows.append((t, values(c)))
	return rows


def integer_csr(rng, n, V, lo, hi):
	"""Values in -8 .. 8 (zeros included: stored zeros take part): every partial sum is an exactly representable integer."""
	return csr_from_rows(_random_rows(rng, n, V, lo, hi, lambda c: rng.integers(-8, 9, c).astype(np.float32)), V)


def real_csr(rng, n, V, lo, hi):
	"""Standard-normal values: the chain's roundings depend on its order."""
	return csr_from_rows(_random_rows(rng, n, V, lo, hi, lambda c: rng.standard_normal(c).astype(np.float32)), V)


def zipf_csr(rng, n, V, per_row, n_common=4, integer=False):
	"""TF-IDF-like: the first n_common terms are in (nearly) every row, the others drawn with probability ~ 1 / rank, so most terms sit in
	a handful of rows.  About per_row terms per row."""
	p = 1.0 / np.arange(1, V - n_common + 1)
	p /= p.sum()
	rows = []
	for _ in range(n):
		common = np.flatnonzero(rng.random(n_common) < 0.97)
		c = min(max(per_row - common.size, 0), V - n_common)
		rare = n_common + rng.choice(V - n_common, size=c, replace=False, p=p) if c else np.zeros(0, dtype=np.int64)
		t = np.sort(np.concatenate([common, rare])).astype(np.int32)
		v = rng.integers(1, 9, t.size).astype(np.float32) if integer else np.abs(rng.standard_normal(t.size)).astype(np.float32) + np.float32(0.01)
		rows.append((t, v))
	return csr_from_rows(rows, V)
