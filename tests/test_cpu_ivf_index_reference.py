"""tests/ivf_index_numpy.py held on its own, without a GPU: the host restatement of the index classes is what tests/test_gpu_ivf_index_exact.py
compares the device with bit for bit, so its pieces are checked against independent statements here.

  * chain_scores against the same fmaf chain as a scalar loop in np.longdouble (64-bit significand: x87 hosts only), and its TwoSum
    precondition against a planted inexact step;
  * renorm_rows_ref against the fp64 normalisation (4 ulp), and on the edge rows whose behaviour the device test pins;
  * train_ref through the k-means objective: with unit centroids both Lloyd steps maximise sum_x <x, c_assign(x)>, so it cannot fall;
  * the shared cases are what their names say: the prototype case has empty lists from iteration 0 on, the sub-sample case sub-samples.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_index_numpy as R  # noqa: E402

F32 = np.float32


def _unit_rows(g, n, d):
	C = g.standard_normal((n, d))
	return (C / np.linalg.norm(C, axis=1, keepdims=True)).astype(F32)


# ------------------------------------------------------------------ chain_scores
@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit significand on this host: nothing wider than fp64 to compare with")
def test_chain_scores_equals_the_scalar_loop_in_longdouble():
	"""Integer rows in [-8, 8] against unit-norm fp32 centroids (the assignment's operands).  In np.longdouble a product (4 + 24 bits) is exact and
	the sum with an fp32 accumulator fits 64 bits on this data, so float32(longdouble step) is the fmaf; the fp64 construction must agree."""
	g = np.random.default_rng(0)
	X, C = g.integers(-8, 9, (9, 70)).astype(F32), _unit_rows(g, 5, 70)
	got = R.chain_scores(X, C.T)
	want = np.zeros((9, 5), dtype=F32)
	for m in range(9):
		for n in range(5):
			acc = F32(0)
			for k in range(70):
				acc = F32(np.longdouble(X[m, k]) * np.longdouble(C[n, k]) + np.longdouble(acc))
			want[m, n] = acc
	assert got.dtype == F32 and np.array_equal(got.view(np.int32), want.view(np.int32))
	assert not np.array_equal(got, (X.astype(np.float64) @ C.T.astype(np.float64)).astype(F32)), "the case does not separate the chain from a once-rounded product"


def test_twosum_check_rejects_a_planted_inexact_step():
	"""1 + 2^-60 is not an fp64 number: the second step of [1, 1] . [1, 2^-60] must be refused, and accepted once the small term is representable."""
	A = np.array([[1, 1]], dtype=F32)
	bad, good = np.array([[1], [2.0 ** -60]], dtype=F32), np.array([[1], [2.0 ** -40]], dtype=F32)
	assert R.inexact_steps(np.array([2.0 ** -60]), np.array([1.0])).all() and not R.inexact_steps(np.array([2.0 ** -40]), np.array([1.0])).any()
	with pytest.raises(R.InexactStep):
		R.chain_scores(A, bad)
	assert R.chain_scores(A, good)[0, 0] == F32(1)                  # (1 + 2^-40 is exact in fp64 and rounds to 1 in fp32)
	assert R.chain_scores(A, bad, check=False)[0, 0] == F32(1)
	with pytest.raises(R.InexactStep):                               # a NaN operand is refused as well
		R.chain_scores(np.array([[np.nan, 1]], dtype=F32), good)
	g = np.random.default_rng(1)                                     # the third fmaf step of a 600-column renormalisation
	with pytest.raises(R.InexactStep):
		R.renorm_rows_ref(g.standard_normal((4, 600)).astype(F32) * np.exp2(g.integers(-30, 30, (4, 600))).astype(F32))


# ------------------------------------------------------------------ renorm_rows_ref
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_renorm_rows_ref_is_within_4_ulp_of_the_fp64_normalisation(d):
	"""Grid values m * 2^-e keep the fmaf steps beyond column 256 exact in fp64.  The sum of squares carries at most 3 + 6 + 2 fp32 roundings."""
	from oracle import gemm_chain as G
	M = G.grid(np.random.default_rng(d), (20, d))
	M[M == 0] = 1
	got = R.renorm_rows_ref(M)
	want = M.astype(np.float64) / np.linalg.norm(M.astype(np.float64), axis=1, keepdims=True)
	assert got.dtype == F32 and got.shape == M.shape
	assert (np.abs(got.astype(np.float64) - want) <= 4 * np.spacing(np.abs(want).astype(F32)).astype(np.float64)).all()


@pytest.mark.parametrize("d", [37, 300])
def test_renorm_rows_ref_on_the_edge_rows(d):
	M, want = R.edge_rows(d)
	got = R.renorm_rows_ref(M)
	assert R.same_bits(got, want).all()
	# the table itself, in words: zero, NaN and underflowing rows unchanged; an overflowing row all zeros; an infinite element NaN, the others 0
	assert np.array_equal(got[0].view(np.int32), M[0].view(np.int32)) and (M[0] == 0).all()
	assert np.array_equal(got[1].view(np.int32), M[1].view(np.int32)) and np.isnan(M[1]).sum() == 1
	assert np.array_equal(got[2].view(np.int32), M[2].view(np.int32)) and (M[2] != 0).all()
	assert (got[3] == 0).all() and np.isfinite(M[3]).all() and (M[3] != 0).all()
	assert np.isnan(got[4][np.isinf(M[4])]).all() and (got[4][~np.isinf(M[4])] == 0).all() and np.isinf(M[4]).sum() == 1
	assert abs(float(np.linalg.norm(got[5].astype(np.float64))) - 1) < 1e-6


# ------------------------------------------------------------------ train_ref
@pytest.mark.parametrize("name", ["d24", "d64", "d130"])
def test_spherical_training_never_lowers_the_objective(name):
	"""F_t = sum_x <x, c_a(x)> in fp64, a = the assignment under the centroids after t iterations.  An iteration without a split replaces every
	centroid by the unit vector that maximises its list's share of F, then every assignment by the maximising list: F cannot fall, up to the
	centroids' rounding -- about a dozen fp32 roundings each, ||delta c|| <= 2^-20, hence 2^-20 sum ||x||."""
	niter = R.NITER
	X, _, info = R.exact_case(name, True, niter)
	Xd = X.astype(np.float64)
	F = [float((Xd * C.astype(np.float64)[R.assign_ref(X, C)]).sum()) for C in info["history"]]
	slack = 2.0 ** -20 * float(np.linalg.norm(Xd, axis=1).sum())
	checked = 0
	for t in range(niter):
		if info["empty"][t] == 0:
			assert F[t + 1] >= F[t] - slack, (t, F)
			checked += 1
	assert checked == niter and F[-1] > F[0]
	for C in info["history"]:
		assert np.abs(np.linalg.norm(C.astype(np.float64), axis=1) - 1).max() < 2.0 ** -20


def test_the_shared_cases_are_what_they_are_named():
	X, C, info = R.exact_case("prototypes", True)
	c = R.CASES["prototypes"]
	assert np.unique(X, axis=0).shape[0] == 8 and (X == 0).all(axis=1).sum() == c["n"] // 8
	assert len(info["empty"]) == R.NITER and info["empty"][0] >= c["nlist"] - 8 and min(info["empty"]) >= c["nlist"] - 8   # empty lists, hence splits, in EVERY iteration
	# iteration 0 on the reference alone: the lists built from the initial centroids
	counts, _, _ = R.build_lists_ref(R.assign_ref(X, info["history"][0]), c["nlist"])
	assert int((counts == 0).sum()) == info["empty"][0] > 0
	assert R.exact_case("prototypes", False)[2]["empty"][0] > 0

	X, C, info = R.exact_case("subsample", True)
	c = R.CASES["subsample"]
	rows = info["subsampled"]
	cap = c["nlist"] * c["max_points_per_centroid"]
	assert rows is not None and rows.shape == (cap,) and cap < c["n"] and (np.diff(rows) > 0).all()
	assert not np.array_equal(rows, np.arange(cap))
	for name in ("d24", "d64", "d130"):
		assert R.exact_case(name, True)[2]["subsampled"] is None


def test_split_follows_split_clusters():
	"""One empty list among three: it takes the heavy list's centroid with the alternating perturbation, the heavy list the mirror image."""
	C = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=F32)
	out = R.split_empty_ref(C, np.array([1, 0, 10]), np.random.default_rng(0))   # weights (0, 0, 9): the draw can only be list 2
	e = F32(1) / F32(1024)
	assert np.array_equal(out[0], C[0])
	assert np.array_equal(out[1], C[2] * np.array([1 + e, 1 - e, 1 + e], dtype=F32))
	assert np.array_equal(out[2], C[2] * np.array([1 - e, 1 + e, 1 - e], dtype=F32))


def test_filter_and_padding_follow_the_faiss_convention():
	vals = np.array([[5, 4, 3, -np.inf]], dtype=F32)
	idx = np.array([[7, 2, 9, -1]], dtype=np.int32)
	D, I = R.filter_ref(vals, idx, [{2}], 3)
	assert D.dtype == F32 and I.dtype == np.int64
	assert I.tolist() == [[7, 9, -1]] and D[0, :2].tolist() == [5, 3] and D[0, 2] == np.finfo(F32).min
	v, i = R.device_form(D, I)
	assert i.dtype == np.int32 and v[0, 2] == -np.inf
