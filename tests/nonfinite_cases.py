"""Host-side operands and references for scores that hold NaN and +-inf (no tests here; tests/fused_exact_cases.py is the precedent).
Used by tests/test_cpu_nonfinite_reference.py and tests/test_gpu_fused_nonfinite.py.

Operands: X [Q x K] integers in [-2, 3], E [K x I] integers in [-3, 3] (float64 arrays; exact in bf16, every finite score an integer
below 2^24), then NaN, +inf or -inf planted in named cells.

Scores: never a BLAS product of arrays that hold NaN or inf.  The class of every cell comes from integer indicator products (exact):
  n_nan  = #{k : a factor is NaN, or one is infinite and the other zero}
  n_pos / n_neg = #{k : the product is +inf / -inf}
  S[q, i] = NaN if n_nan > 0 or (n_pos > 0 and n_neg > 0); else +inf if n_pos > 0; else -inf if n_neg > 0; else the integer product of
  the operands with their non-finite cells zeroed.
A NaN or an infinity, once in a sum, stays whatever is added later, so the class does not depend on the summation order: it holds for any
MFMA shape and any split of K.

Top-k: per row the non-NaN cells by value descending (+inf first, -inf last), ties by ascending row of E^T; rows with fewer than k such
cells are padded with (-inf, -1) -- the order of make_key / sel_finish (csrc/common.hpp, csrc/select.hpp), the wording of
anncur_rowwise_topk in include/anncur_hip.h."""
import numpy as np

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ scores
def _ind(M):
	"""Indicator matrices of a float array: nan, +inf, -inf, zero, finite > 0, finite < 0, and the array with non-finite cells zeroed.
	All float64 holding small integers: their products below are exact (sums below 2^24) and hold no NaN or inf."""
	nan, pinf, ninf = np.isnan(M), M == INF, M == -INF
	fin = ~(nan | pinf | ninf)
	M0 = np.where(fin, M, 0.0)
	assert (M0 == np.rint(M0)).all()
	i64 = lambda a: a.astype(np.float64)
	return i64(nan), i64(pinf), i64(ninf), i64(fin & (M0 == 0)), i64(fin & (M0 > 0)), i64(fin & (M0 < 0)), i64(M0)


def score_classes(X, E):
	"""X [Q x K], E [K x I] (floats holding integers, NaN, +-inf) -> (n_nan, n_pos, n_neg, finite part), int64 [Q x I] each."""
	xn, xp, xm, xz, xpos, xneg, X0 = _ind(np.asarray(X, dtype=np.float64))
	en, ep, em, ez, epos, eneg, E0 = _ind(np.asarray(E, dtype=np.float64))
	K = X0.shape[1]
	assert E0.shape[0] == K and int(np.abs(X0).max(initial=0)) * int(np.abs(E0).max(initial=0)) * K < 1 << 24
	one_x, one_e = np.ones_like(xn), np.ones_like(en)
	n_nan = xn @ one_e + one_x @ en + (xp + xm) @ ez + xz @ (ep + em)
	n_pos = xp @ (epos + ep) + xm @ (eneg + em) + xpos @ ep + xneg @ em
	n_neg = xp @ (eneg + em) + xm @ (epos + ep) + xpos @ em + xneg @ ep
	return tuple(np.rint(a).astype(np.int64) for a in (n_nan, n_pos, n_neg, X0 @ E0))


def scores(X, E):
	"""S [Q x I] float64: NaN, +-inf or the exact integer score (see the module docstring)."""
	n_nan, n_pos, n_neg, fin = score_classes(X, E)
	S = fin.astype(np.float64)
	S[n_neg > 0] = -INF
	S[n_pos > 0] = INF
	S[(n_nan > 0) | ((n_pos > 0) & (n_neg > 0))] = NAN
	return S


# ------------------------------------------------------------------ top-k
def reference_topk(S, k, item_ids=None):
	"""THE top-k of S [Q x I] (float64 with NaN / +-inf) -> (values float32 [Q x k], ids int64 [Q x k], n_valid int64 [Q]).
	Non-NaN cells by value descending, ties by ascending row; (-inf, -1) pads.  item_ids [I]: the ids are mapped afterwards (ties stay
	ordered by row)."""
	Q, I = S.shape
	assert k <= I
	nan = np.isnan(S)
	key = np.where(nan, -INF, S)
	rows = np.broadcast_to(np.arange(I, dtype=np.int64), S.shape)
	order = np.lexsort((rows, -key, nan), axis=-1)[:, :k]          # primary: non-NaN first; then value descending; then row ascending
	n_valid = (~nan).sum(1)
	pad = np.arange(k)[None, :] >= n_valid[:, None]
	val = np.take_along_axis(S, order, axis=1)
	assert not np.isnan(val[~pad]).any() and (np.abs(val[~pad & np.isfinite(val)]) < 1 << 24).all()
	ids = order if item_ids is None else np.asarray(item_ids, dtype=np.int64)[order]
	val = np.where(pad, -INF, val).astype(np.float32)
	return val, np.where(pad, -1, ids).astype(np.int64), n_valid


def kth_non_nan(S, k):
	"""The k-th best non-NaN score per row (float64 [Q]); NaN where the row holds fewer than k."""
	val, ids, n_valid = reference_topk(S, k)
	return np.where(n_valid >= k, val[:, -1].astype(np.float64), NAN)


# ------------------------------------------------------------------ the error kernels' sums
def reference_error_sums(S, A):
	"""err_sq[q] = sum_i (S - A)^2: NaN if the row of S - A holds a NaN, else +inf if it holds an infinity, else the exact integer sum;
	norm_sq[q] = sum_i A^2 from A alone, by the same rule.  Returns (err float64 [Q], nrm float64 [Q])."""
	def sums(D):
		nan = np.isnan(D).any(1)
		inf = np.isinf(D).any(1)
		fin = np.where(np.isfinite(D), D, 0.0)
		s = (fin * fin).sum(1)
		assert (s < 1 << 24).all() and (fin == np.rint(fin)).all()
		return np.where(nan, NAN, np.where(inf, INF, s))
	with np.errstate(invalid="ignore"):
		D = S - A                                   # (inf - inf = NaN, NaN - x = NaN: one subtraction per cell, no order to depend on)
	return sums(D), sums(np.asarray(A, dtype=np.float64))


# ------------------------------------------------------------------ the prepass' threshold
def nan_ignoring_gmax(S, tiles, group_rows):
	"""Group maxima of the sampled tiles as the prepass' fmaxf chains form them: the maximum of the non-NaN cells, NaN for an all-NaN group.
	tiles: the sampled 32-item tiles; group_rows [groups per tile x items per group] (fused_exact_cases.group_rows).  -> float64 [Q x groups]."""
	items = (np.asarray(tiles)[:, None, None] * 32 + np.asarray(group_rows)[None, :, :])
	assert int(items.max()) < S.shape[1]
	G = S[:, items.reshape(-1)].reshape(S.shape[0], -1, group_rows.shape[1])
	return np.fmax.reduce(G, axis=2)


def kth_largest_nan_lowest(G, k):
	"""The k-th largest of each row of G with NaN below everything (kth_value_wave_kernel keys a NaN as 0): NaN if fewer than k non-NaN."""
	nan = np.isnan(G)
	srt = -np.sort(-np.where(nan, -INF, G), axis=1)
	return np.where((~nan).sum(1) >= k, srt[:, k - 1], NAN)


# ------------------------------------------------------------------ cases
CASES = ("nan-items", "nan-queries", "inf-column-3", "inf-column-k+3", "neg-inf-floor", "inf-minus-inf", "few-left", "mixed", "nan-tiles")


def case_queries(name):
	"""Q of a case: 70 = three 32-row sub-tiles, the last ragged; few-left takes 5 (every query of it takes the whole-row rescan)."""
	return 5 if name == "few-left" else 70


class Case:
	"""One problem: X [Q x K], E [K x I] with the plants of `name`, S = scores(X, E), and what the case promises (asserted here, on the host).

	sampled: the 32-item tiles the plan's prepass samples (fused_exact_cases.sample_tiles), so that plants land inside and outside the sample.
	x_nnz: None = dense X; n = at most n random non-zero columns per query besides the planted columns (small scores for the error sums)."""

	def __init__(self, name, Q, I, K, k, sampled, seed=0, x_nnz=None):
		assert name in CASES and K >= 16 and I % 32 == 17 and k + 3 < I
		g = np.random.default_rng([seed, CASES.index(name), I, K, k])
		X = g.integers(-2, 4, (Q, K)).astype(np.float64)
		if x_nnz is not None:
			keep = np.argsort(g.random((Q, K)), axis=1)[:, :x_nnz]
			m = np.zeros((Q, K), dtype=bool)
			np.put_along_axis(m, keep, True, axis=1)
			X = np.where(m, X, 0.0)
		E = g.integers(-3, 4, (K, I)).astype(np.float64)
		self.name, self.Q, self.I, self.K, self.k = name, Q, I, K, k
		sampled = np.unique(np.asarray(sampled, dtype=np.int64))
		unsampled = np.setdiff1d(np.arange(I // 32, dtype=np.int64), sampled)
		assert sampled[0] == 0 and unsampled.size > 0
		c0, c1, c2, c3, cn = 1, K - 2, 5, K // 2, 7          # the columns the plants use
		q = np.arange(Q)
		self.nan_items = np.zeros(0, dtype=np.int64)
		self.nan_queries = np.zeros(0, dtype=np.int64)
		self.notes = {}

		def nan_items():
			self.nan_items = np.array([0, sampled[sampled.size // 2] * 32 + 5, unsampled[unsampled.size // 2] * 32 + 9, I - 1], dtype=np.int64)
			assert np.unique(self.nan_items).size == 4
			X[:, cn] = np.where(X[:, cn] == 0, 1.0, X[:, cn])   # (any factor makes a NaN; kept non-zero so that the column reads the same in every case)
			E[cn, self.nan_items] = NAN

		def nan_queries():
			self.nan_queries = np.array([0, 37, Q - 1], dtype=np.int64)
			X[0, 3], X[37, K - 1], X[Q - 1, K // 2 + 1] = NAN, NAN, NAN

		def inf_column(n):
			X[:, c0] = np.array([2.0, 0.0, -1.0])[q % 3]        # +inf rows, NaN rows (inf . 0), -inf rows
			J = np.sort(np.concatenate([[3, I - 2], g.choice(np.arange(40, I - 40), n - 2, replace=False)]))
			assert np.unique(J).size == n
			E[c0, J] = INF
			self.notes["J"] = J

		def neg_inf_floor(keep):
			X[:, c1] = np.array([1.0, 0.0, -2.0])[(q // 3) % 3]  # a -inf floor, NaN everywhere else, a flood of +inf
			E[c1, :] = -INF
			E[c1, keep] = g.integers(-3, 4, keep.size)
			self.notes["kept"] = keep

		def inf_minus_inf():
			X[:, c2], X[:, c3] = 1.0 + q % 3, 3.0 - q % 2
			both = np.sort(g.choice(np.arange(I), 9, replace=False))
			E[c2, both], E[c3, both] = INF, -INF
			self.notes["both"] = both

		if name == "nan-items":
			nan_items()
		elif name == "nan-queries":
			nan_queries()
		elif name.startswith("inf-column"):
			inf_column(3 if name == "inf-column-3" else k + 3)
		elif name == "neg-inf-floor":
			neg_inf_floor(np.sort(g.choice(np.arange(I), k - 10, replace=False)))
		elif name == "inf-minus-inf":
			inf_minus_inf()
		elif name == "few-left":
			left = np.sort(np.concatenate([[I - 1], g.choice(np.arange(I - 1), 36, replace=False)]))
			assert left.size == 37 < k
			X[:, cn] = np.where(X[:, cn] == 0, 1.0, X[:, cn])
			E[cn, np.setdiff1d(np.arange(I), left)] = NAN
			self.notes["left"] = left
		elif name == "nan-tiles":
			# whole SAMPLED tiles are NaN, k - 10 of the prepass' group maxima with them (8 groups of 4 items per tile: all our plans; with groups
			# of 16 fewer maxima go, which asks less): k non-NaN maxima are left, so tau0 is their k-th.  A threshold kernel that ranked the NaN
			# maxima ABOVE the numbers would return about the 10th largest instead -- above the true k-th score, hidden by the select's rescan
			# unless the fallback counter or the ladder state is read.
			n_t = -(-(k - 10) // 8)
			assert 8 * (sampled.size - n_t) >= k
			t = sampled[np.sort(g.choice(np.arange(1, sampled.size), n_t, replace=False))]
			self.nan_items = (t[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)
			X[:, cn] = np.where(X[:, cn] == 0, 1.0, X[:, cn])
			E[cn, self.nan_items] = NAN
		else:   # mixed: every plant in one problem; the floor on every second item, so that the other plants still show
			nan_items()
			nan_queries()
			inf_column(3)
			neg_inf_floor(np.arange(0, I, 2))
			inf_minus_inf()
		self.X, self.E = X, E
		self.S = scores(X, E)
		self._promises(c0, c1)

	def _promises(self, c0, c1):
		"""What the issue expects of each case, checked on the reference itself."""
		S, k, Q, I, name = self.S, self.k, self.Q, self.I, self.name
		val, ids, n_valid = reference_topk(S, k)
		q = np.arange(Q)
		if name == "nan-items":
			assert np.isnan(S[:, self.nan_items]).all() and np.isnan(S).sum() == 4 * Q and not np.isin(ids, self.nan_items).any() and (n_valid == I - 4).all()
		if name == "nan-tiles":
			assert np.isnan(S[:, self.nan_items]).all() and np.isnan(S).sum() == self.nan_items.size * Q and not np.isin(ids, self.nan_items).any() and (n_valid >= k).all()
		if name == "nan-queries":
			assert np.isnan(S[self.nan_queries]).all() and np.isnan(S).sum() == 3 * I and (ids[self.nan_queries] == -1).all() and np.isfinite(val[np.setdiff1d(q, self.nan_queries)]).all()
		if name.startswith("inf-column"):
			J = self.notes["J"]
			up, mid, down = q % 3 == 0, q % 3 == 1, q % 3 == 2
			assert (S[np.ix_(up, J)] == INF).all() and np.isnan(S[np.ix_(mid, J)]).all() and (S[np.ix_(down, J)] == -INF).all()
			n = min(k, J.size)
			assert (ids[up, :n] == J[None, :n]).all() and (val[up, :n] == INF).all() and not np.isin(ids[~up], J).any()
		if name == "neg-inf-floor":
			kept, m = self.notes["kept"], k - 10
			floor, none, flood = (q // 3) % 3 == 0, (q // 3) % 3 == 1, (q // 3) % 3 == 2
			rest = np.setdiff1d(np.arange(I), kept)
			assert np.isin(ids[floor, :m], kept).all() and (val[floor, m:] == -INF).all() and (ids[floor, m:] == rest[None, :10]).all()
			assert (n_valid[none] == m).all() and (ids[none, m:] == -1).all() and np.isin(ids[none, :m], kept).all()
			assert (val[flood] == INF).all() and (ids[flood] == rest[None, :k]).all()
		if name == "inf-minus-inf":
			assert np.isnan(S[:, self.notes["both"]]).all() and np.isnan(S).sum() == 9 * Q
		if name == "few-left":
			assert (n_valid == 37).all() and (np.sort(ids[:, :37], axis=1) == self.notes["left"][None, :]).all() and (ids[:, 37:] == -1).all()
		if name == "mixed":
			cls = [np.isnan(S).any(), (S == INF).any(), (S == -INF).any(), (n_valid < k).any(), (n_valid >= k).any()]
			assert all(cls), cls


def with_low_parts(M, seed):
	"""float32 copy of an operand with non-zero low parts for the split-bf16 route: every finite cell gets m 2^-12, m in {-3..3} \\ {0} (far below
	half a bf16 ulp of any non-zero integer here, so hi = the integer and lo = m 2^-12; a zero cell becomes m 2^-12 itself, hi = that, lo = 0)."""
	g = np.random.default_rng(seed)
	m = g.integers(1, 4, M.shape) * (2 * g.integers(0, 2, M.shape) - 1)
	with np.errstate(invalid="ignore"):
		return np.where(np.isfinite(M), M + m * 2.0 ** -12, M).astype(np.float32)
