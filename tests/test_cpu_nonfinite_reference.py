"""The host reference for NaN and +-inf scores (tests/nonfinite_cases.py) against independent statements of the same thing; no device.
  - the class algebra (integer indicator products) against a scalar float32 loop that accumulates the same products in two k orders,
    on shapes of a few dozen cells that hold every combination of factor classes;
  - the top-k reference against torch.topk on NaN-free rows with distinct values, and its order and padding on rows with NaN, +-inf and ties;
  - the error sums' classes, the prepass threshold helpers, and that every case builds and keeps its own promises."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_cases as nf  # noqa: E402

NAN, INF = nf.NAN, nf.INF
_VALUES = [NAN, INF, -INF, 0.0, 2.0, -3.0]


def _scalar_f32(X, E, order):
	out = np.empty((X.shape[0], E.shape[1]), dtype=np.float32)
	with np.errstate(invalid="ignore", over="ignore"):
		for q in range(X.shape[0]):
			for i in range(E.shape[1]):
				acc = np.float32(0)
				for kk in order:
					acc = np.float32(acc + np.float32(X[q, kk]) * np.float32(E[kk, i]))
				out[q, i] = acc
	return out


def _same(a, b):
	a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
	return bool((np.isnan(a) == np.isnan(b)).all() and (a[~np.isnan(a)] == b[~np.isnan(b)]).all())


def test_every_pair_of_factor_classes_k1():
	"""K = 1: the 6 x 6 table of single products."""
	X = np.array(_VALUES)[:, None]
	E = np.array(_VALUES)[None, :]
	S = nf.scores(X, E)
	assert _same(S, _scalar_f32(X, E, [0]))
	assert np.isnan(S[1, 3]) and np.isnan(S[3, 2]) and S[1, 2] == -INF and S[2, 2] == INF and S[4, 5] == -6 and np.isnan(S[0, 3])


@pytest.mark.parametrize("seed", range(6))
def test_class_algebra_against_a_scalar_float32_loop_in_two_orders(seed):
	"""K = 4, a few dozen cells: every row of X and column of E draws its cells from all six classes, so sums meet inf + inf, inf - inf,
	NaN + inf and finite + inf.  Forward and reverse k order agree with each other and with the algebra."""
	g = np.random.default_rng(seed)
	Q, K, I = 6, 4, 7
	X = np.array(_VALUES)[g.integers(0, 6, (Q, K))]
	E = np.array(_VALUES)[g.integers(0, 6, (K, I))]
	X[0], E[:, 0] = [2.0, -3.0, 0.0, 2.0], [-3.0, 2.0, 2.0, 0.0]    # one finite row and column at least
	X[1], E[:, 1] = [2.0, 2.0, 0.0, 0.0], [INF, -INF, 2.0, NAN]      # inf - inf; a NaN against a zero
	S = nf.scores(X, E)
	fwd, rev = _scalar_f32(X, E, range(K)), _scalar_f32(X, E, range(K - 1, -1, -1))
	assert _same(fwd, rev) and _same(S, fwd)
	assert S[0, 0] == -12 and np.isnan(S[1, 1]) and np.isnan(S[0, 1])   # (0 . NaN: NaN)
	seen = [np.isnan(S).any(), np.isfinite(S).any()]
	assert all(seen)


def test_topk_reference_equals_torch_topk_on_distinct_nan_free_rows():
	g = np.random.default_rng(1)
	S = np.stack([g.permutation(500) - 250 for _ in range(9)]).astype(np.float64)
	val, ids, n_valid = nf.reference_topk(S, 40)
	tv, ti = torch.topk(torch.from_numpy(S), 40, dim=1)
	assert np.array_equal(val, tv.numpy().astype(np.float32)) and np.array_equal(ids, ti.numpy()) and (n_valid == 500).all()


def test_topk_reference_order_ties_and_padding():
	S = np.array([[1.0, NAN, INF, -INF, 1.0, INF, NAN, -INF, 0.0],
				  [NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN],
				  [NAN, -INF, NAN, NAN, 5.0, NAN, NAN, NAN, NAN]])
	val, ids, n_valid = nf.reference_topk(S, 8)
	assert n_valid.tolist() == [7, 0, 2]
	assert ids[0].tolist() == [2, 5, 0, 4, 8, 3, 7, -1] and val[0].tolist() == [INF, INF, 1.0, 1.0, 0.0, -INF, -INF, -INF]
	assert (ids[1] == -1).all() and (val[1] == -INF).all()
	assert ids[2].tolist() == [4, 1] + [-1] * 6 and val[2].tolist() == [5.0] + [-INF] * 7
	# a real -inf cell comes before a pad and keeps its row; ids map afterwards, ties stay ordered by row
	perm = np.array([8, 7, 6, 5, 4, 3, 2, 1, 0])
	_, mapped, _ = nf.reference_topk(S, 8, item_ids=perm)
	assert mapped[0].tolist() == [6, 3, 8, 4, 0, 5, 1, -1]
	kth = nf.kth_non_nan(S, 2)
	assert kth[0] == INF and np.isnan(kth[1]) and kth[2] == -INF


def test_error_sums_by_class():
	S = np.array([[1.0, 2.0, 3.0], [1.0, NAN, 3.0], [INF, 2.0, 3.0], [INF, NAN, 0.0], [INF, 0.0, 0.0], [1.0, 1.0, 1.0]])
	A = np.array([[0.0, 2.0, 5.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [INF, 0.0, 0.0], [-INF, NAN, 2.0]])
	err, nrm = nf.reference_error_sums(S, A)
	assert err[0] == 5 and np.isnan(err[1]) and err[2] == INF and np.isnan(err[3]) and np.isnan(err[4]) and np.isnan(err[5])
	assert nrm[:4].tolist() == [29, 14, 14, 14] and nrm[4] == INF and np.isnan(nrm[5])


def test_threshold_helpers():
	S = np.full((2, 64), 1.0)
	S[0, :4], S[0, 4], S[1, :] = NAN, 7.0, NAN
	S[1, 40] = -INF
	rows = np.arange(32).reshape(8, 4)
	G = nf.nan_ignoring_gmax(S, np.array([0, 1]), rows)
	assert G.shape == (2, 16) and np.isnan(G[0, 0]) and G[0, 1] == 7 and np.isnan(G[1, :10]).all() and G[1, 10] == -INF
	t = nf.kth_largest_nan_lowest(G, 15)
	assert t[0] == 1 and np.isnan(t[1])
	assert np.isnan(nf.kth_largest_nan_lowest(G, 16)).all()


@pytest.mark.parametrize("name", nf.CASES)
def test_every_case_builds_and_keeps_its_promises(name):
	"""At a small stand-in shape (the GPU tests build the cases at the plans' shapes): the constructor asserts what the case promises."""
	I, K, k = 40 * 32 + 17, 24, 50
	sampled = np.arange(0, 40, 2)
	c = nf.Case(name, nf.case_queries(name), I, K, k, sampled)
	assert c.S.shape == (c.Q, I)
	lo = nf.with_low_parts(c.X, 3)
	assert lo.dtype == np.float32 and (np.isnan(lo) == np.isnan(c.X)).all() and (lo[np.isfinite(lo)] != c.X[np.isfinite(c.X)]).all()
	hi = torch.from_numpy(lo).bfloat16().float().numpy()
	fin = np.isfinite(c.X) & (c.X != 0)
	assert (hi[fin] == c.X[fin]).all()   # the low part stays below half a bf16 ulp: hi is the integer

