"""anncur_amd.search end to end on tie-free integer data: ids and values equal, no tolerance.

The data is that of tests/test_gpu_filtered_routes.py (built here the same way): query q reads two embedding columns of its own,
X[q, 2q] = 64, X[q, 2q + 1] = 1, and item i holds there the two digits of a code that is a permutation of range(I) per query, so
S[q, i] = 64 hi + lo is a distinct integer along every row (hi centred on 0 for the case's item count), every operand exact in bf16,
every partial sum an integer below 2^24.  The CUR index is built over an identity anchor block (R[:, anc] = 1, so U = 1 and the index'
E^T is R^T itself): the approximate scores ARE S, and S[:, anc] = X.  The exact matrix the scorer answers from is A = S as fp32 (test (d) moves one row of it away from S).

The item count is the smallest at which the fused route takes the retrieval of the case -- k_retvr + 200 excluded anchors -- found on the
host with ops.fused_supported, plus a ragged tail; every test asserts the route it runs.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, K_TOP, K_RETVR, N_ANC = 33, 10, 32, 200
I_MAX = 256 * 64          # the two-digit code covers this many items
TAIL = 27
DTYPES = ("bf16", "fp32", "bf16x3")


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _sweep_k(ops, compute_dtype, I, excluded):
	"""(Kp, candidates the fused sweep is asked for) of CURRowIndex.topk(X, K_RETVR) with `excluded` items per query left out."""
	if compute_dtype == "bf16":
		return ops.padded_k(N_ANC), K_RETVR + excluded
	return ops.split_kp(N_ANC), ops.split_candidates(I, K_RETVR, n_excl=excluded)


@functools.lru_cache(maxsize=None)
def _item_count(compute_dtype):
	"""The smallest item count (a multiple of 64, plus the tail) at which the fused path takes both retrievals of the case -- plain and
	with the 200 anchors excluded -- from the plan query on the host.  The dense fp32 route has no such threshold: it takes the bf16 one's."""
	from anncur_amd import ops
	dt = "bf16" if compute_dtype == "fp32" else compute_dtype
	for I in range(1024, I_MAX - TAIL, 64):
		if all(ops.fused_supported(Q, I, *_sweep_k(ops, dt, I, e)) for e in (0, N_ANC)):
			return I + TAIL
	raise AssertionError("no item count up to 2^14 takes the fused path")


@functools.lru_cache(maxsize=None)
def _case(I, K=N_ANC):
	"""(X [Q x K] float32, R [K x I] float32 anchor rows with the identity anchor block, anc [K] ascending, S [Q x I] int64 = X . R)."""
	assert K >= 2 * Q and I <= I_MAX
	rng = np.random.default_rng(I + K)
	code = np.stack([rng.permutation(I) for _ in range(Q)])
	X = np.zeros((Q, K), dtype=np.float32)
	E = np.zeros((I, K), dtype=np.float32)
	q = np.arange(Q)
	X[q, 2 * q], X[q, 2 * q + 1] = 64, 1
	E[:, 0:2 * Q:2], E[:, 1:2 * Q:2] = (code // 64 - I // 128).T, (code % 64).T           # (hi centred for THIS item count: the best scores are far above the anchors' 64)
	anc = np.sort(rng.choice(I, K, replace=False))
	R = E.T.copy()
	R[:, anc] = np.eye(K, dtype=np.float32)
	S = torch.from_numpy(X.astype(np.int64) @ R.astype(np.int64))
	non_anchor = np.setdiff1d(np.arange(I), anc)
	assert all(np.unique(r[non_anchor]).size == non_anchor.size for r in S.numpy())   # tie-free outside the anchors
	assert np.array_equal(S.numpy()[:, anc], X.astype(np.int64))
	return X, R, anc, S


@functools.lru_cache(maxsize=None)
def _index(compute_dtype):
	from anncur_amd import ops
	from anncur_amd.cur import CURRowIndex
	I = _item_count(compute_dtype)
	X, R, anc, S = _case(I)
	Rd = torch.from_numpy(R).cuda()
	if compute_dtype == "bf16": Rd = Rd.bfloat16()
	index = CURRowIndex(Rd, anc, compute_dtype=compute_dtype, pinv_backend="numpy")
	assert torch.equal(index._Et.float().cpu(), torch.from_numpy(R.T.copy())), "the case needs U = identity exactly"
	A = S.float().cuda().contiguous()
	return index, A, anc, S


def _assert_route(ops, index, compute_dtype, excl):
	"""The route CURRowIndex.topk(X, K_RETVR, exclude=excl) takes, asserted from the plan queries and from what the index built."""
	I, e = index.m, excl.e_max if excl is not None else 0
	if compute_dtype == "fp32":
		assert index._Etp is None and index._split is None          # the dense fp32 route
		return
	Kp, kc = _sweep_k(ops, compute_dtype, I, e)
	assert ops.fused_supported(Q, I, Kp, kc), "the case left the fused path"
	if e:
		assert not ops.fused_supported(Q, I - TAIL - 64, Kp, kc) or not ops.fused_supported(Q, I - TAIL - 64, *_sweep_k(ops, compute_dtype, I - TAIL - 64, 0)), "a smaller item count would do"
	if compute_dtype == "bf16":
		assert index._Etp is not None and index._Etp.shape[1] == Kp
	else:
		assert index._split is not None and index._split.kp == Kp and index._split.takes(Q, I, K_RETVR, excl)


def _pool_reference(A_cpu, S, anc, k, k_retvr):
	"""torch.topk on the CPU of A (float64) with every cell outside anchors + retrieved at -inf; the retrieved set is the brute-force top
	k_retvr of the CPU score matrix S with the anchors excluded.  Ties (anchor scores only) by the smaller id."""
	I = S.shape[1]
	Sx = S.double().clone()
	Sx[:, torch.from_numpy(anc)] = -np.inf
	retrieved = torch.topk(Sx, k_retvr, dim=1).indices                       # tie-free outside the anchors
	keep = torch.zeros(S.shape, dtype=torch.bool)
	keep[:, torch.from_numpy(anc)] = True
	keep.scatter_(1, retrieved, True)
	Ap = torch.where(keep, A_cpu.double(), torch.tensor(-np.inf, dtype=torch.float64))
	key = Ap * (1 << 15) - torch.arange(I, dtype=torch.float64)               # |A| < 2^15, I < 2^15: exact in fp64
	ids = torch.topk(key, k, dim=1).indices
	vals = torch.gather(Ap, 1, ids)
	assert torch.isfinite(vals).all()
	return vals.float().numpy(), ids.numpy(), retrieved.numpy()


def _equal(res, want_v, want_i, what):
	got_v, got_i = res.values.cpu().numpy(), res.indices.cpu().numpy().astype(np.int64)
	assert res.values.dtype == torch.float32 and res.indices.dtype == torch.int32
	bad = np.nonzero((got_i != want_i).any(1) | (got_v.view(np.int32) != np.asarray(want_v, dtype=np.float32).view(np.int32)).any(1))[0]
	assert bad.size == 0, f"{what}: {bad.size} queries differ, first q={bad[0]}\n got  {got_i[bad[0]]}\n want {want_i[bad[0]]}\n got  {got_v[bad[0]]}\n want {want_v[bad[0]]}"


class CountingScorer(object):
	def __init__(self, scorer):
		self.scorer, self.calls = scorer, []

	def __call__(self, query_ids, item_ids):
		self.calls.append((np.asarray(query_ids).copy(), item_ids.detach().cpu().numpy().copy(), item_ids.dtype, item_ids.is_cuda))
		return self.scorer(query_ids, item_ids)


@pytest.mark.parametrize("compute_dtype", DTYPES)
def test_plain_mode_equals_the_matrix_rerank(ops, compute_dtype):
	"""(a) anchors_in_pool=False with MatrixScorer(A) = ops.rerank(A, index.topk(X, k_retvr).indices, k_retvr, k), bit for bit."""
	from anncur_amd.search import CrossEncoderSearcher, MatrixScorer
	index, A, anc, S = _index(compute_dtype)
	qids = np.arange(Q, dtype=np.int64)
	X = ops.gather_cols(A, anc)
	approx = index.topk(X, K_RETVR)
	_assert_route(ops, index, compute_dtype, None)
	want = ops.rerank(A, approx.indices, K_RETVR, K_TOP)
	got = CrossEncoderSearcher(index, MatrixScorer(A), anchors_in_pool=False).search(qids, K_TOP, K_RETVR)
	assert got.n_scored == K_RETVR
	assert torch.equal(got.indices, want.indices) and torch.equal(got.values.view(torch.int32), want.values.view(torch.int32))
	# a subset of the query rows, in another order: the scorer gathers them
	sub = np.array([7, 0, 32, 5], dtype=np.int64)
	got = CrossEncoderSearcher(index, MatrixScorer(A), anchors_in_pool=False).search(sub, K_TOP, K_RETVR)
	assert torch.equal(got.indices, want.indices[torch.from_numpy(sub).cuda()]) and torch.equal(got.values, want.values[torch.from_numpy(sub).cuda()])


@pytest.mark.parametrize("compute_dtype", DTYPES)
def test_pool_mode_equals_cpu_topk_over_anchors_and_retrieved(ops, compute_dtype):
	"""(b) the CPU reference, and (c) the calls a counting scorer sees."""
	from anncur_amd.search import CrossEncoderSearcher, MatrixScorer
	index, A, anc, S = _index(compute_dtype)
	qids = np.arange(Q, dtype=np.int64)
	scorer = CountingScorer(MatrixScorer(A))
	searcher = CrossEncoderSearcher(index, scorer)
	_assert_route(ops, index, compute_dtype, searcher._excl)
	assert searcher._excl.e_max == N_ANC and searcher._excl.off is None and searcher._shared.n == N_ANC
	got = searcher.search(qids, K_TOP, K_RETVR)
	want_v, want_i, retrieved = _pool_reference(A.cpu(), S, anc, K_TOP, K_RETVR)
	_equal(got, want_v, want_i, f"pool mode {compute_dtype}")
	# (c) two calls: the anchors as ONE shared list, then the per-query candidates -- none of them an anchor
	assert got.n_scored == N_ANC + K_RETVR
	assert len(scorer.calls) == 2
	(q0, items0, dt0, cuda0), (q1, items1, dt1, cuda1) = scorer.calls
	assert np.array_equal(q0, qids) and np.array_equal(q1, qids)
	assert items0.shape == (N_ANC,) and np.array_equal(items0, anc) and dt0 == torch.int32 and cuda0
	assert items1.shape == (Q, K_RETVR) and dt1 == torch.int32 and cuda1
	assert not np.isin(items1, anc).any()
	assert all(set(items1[q]) == set(retrieved[q]) for q in range(Q))
	# the same searcher again: nothing is rebuilt, the result is the same
	again = searcher.search(qids, K_TOP, K_RETVR)
	assert torch.equal(again.indices, got.indices) and torch.equal(again.values, got.values) and len(scorer.calls) == 4
	# k up to the whole pool: the anchors' tied scores (0) come out in id order, then the rest
	full = searcher.search(qids, N_ANC + K_RETVR, K_RETVR)
	fv, fi, _ = _pool_reference(A.cpu(), S, anc, N_ANC + K_RETVR, K_RETVR)
	_equal(full, fv, fi, f"pool mode {compute_dtype}, k = pool")


@pytest.mark.parametrize("compute_dtype", DTYPES)
def test_an_anchor_that_is_the_exact_best_item(ops, compute_dtype):
	"""(d) In row 3 the exact scores of all non-anchor items drop by 20000 and one anchor (an embedding column no query reads, so the
	approximate scores of the other items stay S) scores 100: it is the row's exact best item, its approximate score 100 is far below the
	k_retvr best approximate scores, so the plain mode misses it and the pool mode returns it at rank 0."""
	from anncur_amd.search import CrossEncoderSearcher, MatrixScorer
	index, A, anc, S = _index(compute_dtype)
	qids = np.arange(Q, dtype=np.int64)
	q, j = 3, N_ANC - 1
	assert j >= 2 * Q
	star = int(anc[j])
	Ad = A.clone()
	non_anchor = torch.from_numpy(np.setdiff1d(np.arange(index.m), anc)).cuda()
	Ad[q, non_anchor] -= 20000
	Ad[q, star] = 100
	assert int(Ad[q].argmax()) == star and int((S[q] > 100).sum()) > K_RETVR
	plain = CrossEncoderSearcher(index, MatrixScorer(Ad), anchors_in_pool=False).search(qids, K_TOP, K_RETVR)
	pool = CrossEncoderSearcher(index, MatrixScorer(Ad)).search(qids, K_TOP, K_RETVR)
	assert star not in plain.indices[q].tolist()
	assert int(pool.indices[q, 0]) == star and float(pool.values[q, 0]) == 100.0
	Sd = S.clone()
	Sd[q, star] = 100                                                          # the approximate scores: X[q, j] = 100 moves only the anchor's own
	want_v, want_i, _ = _pool_reference(Ad.cpu(), Sd, anc, K_TOP, K_RETVR)
	_equal(pool, want_v, want_i, f"planted anchor {compute_dtype}")
	want = ops.rerank(Ad, index.topk(ops.gather_cols(Ad, anc), K_RETVR).indices, K_RETVR, K_TOP)
	assert torch.equal(plain.indices, want.indices) and torch.equal(plain.values, want.values)


def test_limits_raise(ops):
	"""(e) k_retvr + kc > MAX_TOPK: the ValueError of ops.filtered_k, before the scorer is called; k beyond the pool."""
	from anncur_amd.search import CrossEncoderSearcher, MatrixScorer
	index, A, anc, S = _index("bf16")
	qids = np.arange(Q, dtype=np.int64)
	scorer = CountingScorer(MatrixScorer(A))
	searcher = CrossEncoderSearcher(index, scorer)
	with pytest.raises(ValueError, match=r"1849 \+ 200 = 2049 candidates per query.*min\(\d+, 2048\) = 2048.*rebuild the index without those items"):
		searcher.search(qids, K_TOP, 2049 - N_ANC)
	with pytest.raises(ValueError, match=r"min\(232, 2048\) = 232"):
		searcher.search(qids, 233, K_RETVR)
	with pytest.raises(ValueError, match=r"min\(32, 2048\) = 32"):
		CrossEncoderSearcher(index, scorer, anchors_in_pool=False).search(qids, 33, K_RETVR)
	assert scorer.calls == []
	from anncur_amd.cur import CURRowIndex
	with pytest.raises(ValueError, match="strictly ascending"):
		unsorted = CURRowIndex.__new__(CURRowIndex)
		unsorted.R, unsorted.m, unsorted.col_idxs = index.R, index.m, anc[::-1].copy()
		CrossEncoderSearcher(unsorted, scorer)
