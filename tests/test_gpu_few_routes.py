"""The small_batch switch of the index classes: CURRowIndex.topk, CURApprox.topk_in_row, FlatIPIndex.search and the adaptive
search's rounds take the small-batch route ("bf16-few") for up to 64 queries when the index was built with small_batch=True, and nothing
changes without it.

Data as in tests/test_gpu_scorer_search.py: query q reads two embedding columns of its own, X[q, 2q] = 64 and X[q, 2q + 1] = 1, and item i
holds there the two digits of a code that is a permutation of the items per query, so S[q, i] = 64 hi + lo is a distinct integer along every
row, every operand exact in bf16.  The CUR indices are built over an identity anchor block (R[:, anc] = 1: U = 1, E^T = R^T), so their
approximate scores ARE S = X . R; the flat index holds the item embeddings themselves.  References are torch.topk on the CPU with the
excluded items at -inf: tie-free among everything a result can hold, so ids and values are compared without tolerance."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
QMAX, K, I, K_TOP = 65, 200, 8219, 10


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=None)
def _case():
	rng = np.random.default_rng(1)
	code = np.stack([rng.permutation(I) for _ in range(QMAX)])
	X = np.zeros((QMAX, K), dtype=np.float32)
	E = np.zeros((I, K), dtype=np.float32)
	q = np.arange(QMAX)
	X[q, 2 * q], X[q, 2 * q + 1] = 64, 1
	E[:, 0:2 * QMAX:2], E[:, 1:2 * QMAX:2] = (code // 64 - I // 128).T, (code % 64).T
	anc = np.sort(rng.choice(I, K, replace=False))
	R = E.T.copy()
	R[:, anc] = np.eye(K, dtype=np.float32)
	return X, E, R, anc


def _reference(S, k, excluded=None):
	"""S [Q x I] int64 -> (values, ids) of the k best per row with the excluded ids (a list per query) left out."""
	Sx = S.double().clone()
	if excluded is not None:
		for q, ids in enumerate(excluded):
			Sx[q, torch.as_tensor(np.asarray(ids, dtype=np.int64))] = -np.inf
	v, i = torch.topk(Sx, k, dim=1)
	assert torch.isfinite(v).all() and (v[:, :-1] > v[:, 1:]).all(), "the case is tie-free where it matters"
	return v.float(), i


def _equal(got_v, got_i, want, what):
	gv, gi = torch.as_tensor(np.asarray(got_v.cpu() if torch.is_tensor(got_v) else got_v)), torch.as_tensor(np.asarray(got_i.cpu() if torch.is_tensor(got_i) else got_i))
	assert torch.equal(gi.long(), want[1]), what + ": ids"
	assert torch.equal(gv.float().view(torch.int32), want[0].view(torch.int32)), what + ": values"


def _exclusions(Q, anc):
	"""None, one shared list (the anchors) and per-query lists of different lengths that hold each query's best items."""
	X, E, R, _ = _case()
	S = torch.from_numpy(X[:Q].astype(np.int64) @ R.astype(np.int64))
	best = torch.topk(S.double(), 7, dim=1).indices.numpy()
	per_query = [sorted(set(best[q, :1 + q % 7].tolist()) | {int(anc[q % K])}) for q in range(Q)]
	return [("none", None, None), ("shared", [int(a) for a in anc], [anc] * Q), ("per-query", per_query, per_query)]


def _cur_row_index(small_batch):
	from anncur_amd.cur import CURRowIndex
	X, E, R, anc = _case()
	index = CURRowIndex(torch.from_numpy(R).cuda().bfloat16(), anc, compute_dtype="bf16", pinv_backend="numpy", small_batch=small_batch)
	assert torch.equal(index._Et.float().cpu(), torch.from_numpy(R.T.copy())), "the case needs U = identity exactly"
	return index


def _cur_approx(small_batch):
	from anncur_amd.cur import CURApprox
	X, E, R, anc = _case()
	return CURApprox(rows=torch.from_numpy(R).cuda().bfloat16(), cols=torch.eye(K).cuda().bfloat16(), row_idxs=np.arange(K), col_idxs=anc, approx_preference="rows",
					 compute_dtype="bf16", pinv_backend="numpy", small_batch=small_batch)


def _flat(small_batch):
	from anncur_amd.nearest_nbr import FlatIPIndex
	X, E, R, anc = _case()
	index = FlatIPIndex(K, dtype="bf16", small_batch=small_batch)
	index.add(E)
	return index


KINDS = {"CURRowIndex": (_cur_row_index, lambda ix, X, k, ex: tuple(ix.topk(X, k, exclude=ex)), lambda ix, Q, k, ex: ix.topk_route(Q, k, ex), "R"),
		 "CURApprox": (_cur_approx, lambda ix, X, k, ex: tuple(ix.topk_in_row(X, k, exclude=ex)), lambda ix, Q, k, ex: ix.topk_route(Q, k, ex), "R"),
		 "FlatIPIndex": (_flat, lambda ix, X, k, ex: ix.search(X.cpu().numpy(), k, exclude=ex), lambda ix, Q, k, ex: ix.search_route(Q, k, ex), "E")}


@pytest.mark.parametrize("kind", list(KINDS))
def test_small_batch_route_of_the_index_classes(ops, kind):
	build, topk, route, operand = KINDS[kind]
	X, E, R, anc = _case()
	items = R if operand == "R" else E.T
	on, off = build(True), build(False)
	assert on.small_batch and not off.small_batch
	for Q in (1, 33, 64, 65):
		Xd = torch.from_numpy(X[:Q]).cuda()
		S = torch.from_numpy(X[:Q].astype(np.int64) @ items.astype(np.int64))
		for name, excl, lists in _exclusions(Q, anc):
			r_on, r_off = route(on, Q, K_TOP, excl), route(off, Q, K_TOP, excl)
			assert r_off in ("bf16", "dense"), (kind, Q, name, r_off)
			assert r_on == ("bf16-few" if Q <= 64 else r_off), (kind, Q, name, r_on)
			want = _reference(S, K_TOP, lists)
			_equal(*topk(on, Xd, K_TOP, excl), want, f"{kind} small_batch=True Q={Q} exclude={name}")
			_equal(*topk(off, Xd, K_TOP, excl), want, f"{kind} small_batch=False Q={Q} exclude={name}")


def test_other_compute_dtypes_ignore_the_flag(ops):
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.nearest_nbr import FlatIPIndex
	X, E, R, anc = _case()
	for dt in ("fp32", "bf16x3"):
		index = CURRowIndex(torch.from_numpy(R).cuda(), anc, compute_dtype=dt, pinv_backend="numpy", small_batch=True)
		plain = CURRowIndex(torch.from_numpy(R).cuda(), anc, compute_dtype=dt, pinv_backend="numpy")
		assert index.topk_route(3, K_TOP) == plain.topk_route(3, K_TOP) != "bf16-few"
		flat = FlatIPIndex(K, dtype=dt, small_batch=True)
		flat.add(E)
		assert flat.search_route(3, K_TOP) != "bf16-few"
	S = torch.from_numpy(X[:3].astype(np.int64) @ R.astype(np.int64))
	_equal(*index.topk(torch.from_numpy(X[:3]).cuda(), K_TOP), _reference(S, K_TOP), "bf16x3 with the flag")


def test_adaptive_search_rounds_take_the_route_and_keep_the_pool(ops):
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	X, E, R, anc = _case()
	A = torch.from_numpy(X[:3].astype(np.int64) @ R.astype(np.int64)).float().cuda().contiguous()
	res = {}
	for flag in (False, True):
		index = _cur_row_index(flag)
		res[flag] = AdaptiveSearcher(index, MatrixScorer(A)).search(np.arange(3), K_TOP, 16, 2, trace=True)
		routes = [t["route"] for t in res[flag].trace if "route" in t]      # (the last entry is the final scored set: no retrieval)
		assert len(routes) == 1 and all((r == "bf16-few") == flag for r in routes), (flag, routes)
		assert index.adaptive_operand().small_batch == flag
	assert torch.equal(res[True].indices, res[False].indices) and torch.equal(res[True].values.view(torch.int32), res[False].values.view(torch.int32))
	assert res[True].n_scored == res[False].n_scored
	for a, b in zip(res[True].trace, res[False].trace):
		assert torch.equal(torch.sort(a["ids"], dim=1).values, torch.sort(b["ids"], dim=1).values), "the rounds scored the same items"
