"""AdaptiveSearcher(incremental=True, seed_shared=...) end to end, in the small fp32 setting of
tests/test_gpu_adaptive_incremental.py: A = U V / sqrt(12) + 0.4 N, Q = 48 test queries, m = 6000 items, kq = 256 anchor queries, 24 (and 25: a
prefix that is no multiple of 16) anchor items, k_step = 12, MatrixScorer.

Seeding the state with the anchors' shared block changes which call factors it, not what any round computes: with the switch on and off
the search returns the same values, indices and n_fallback, and every round's W and status are the same bits.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, K_TOP, RANK = 48, 10, 12
M, KQ, K_STEP, NOISE, SEED = 6000, 256, 12, 0.4, 1


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=None)
def _matrices():
	rng = np.random.default_rng(SEED)
	U, V = rng.standard_normal((KQ + Q, RANK)), rng.standard_normal((RANK, M))
	A = (U @ V / np.sqrt(RANK) + NOISE * rng.standard_normal((KQ + Q, M))).astype(np.float32)
	return torch.from_numpy(A[:KQ].copy()).cuda(), torch.from_numpy(A[KQ:].copy()).cuda()


@functools.lru_cache(maxsize=None)
def _setup(kc):
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import MatrixScorer
	R, At = _matrices()
	anc = np.sort(np.random.default_rng(SEED + 1).choice(M, kc, replace=False))
	return CURRowIndex(R, anc, compute_dtype="fp32", pinv_backend="numpy"), MatrixScorer(At), anc


def _bits(t):
	return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("n_rounds", [2, 4])
@pytest.mark.parametrize("kc", [24, 25])
def test_seeded_and_unseeded_searches_are_the_same_bits(ops, kc, n_rounds):
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, anc = _setup(kc)
	qids = torch.arange(Q, dtype=torch.int64)
	seeded = AdaptiveSearcher(index, scorer, incremental=True, seed_shared=True)
	plain = AdaptiveSearcher(index, scorer, incremental=True, seed_shared=False)
	assert seeded.seed_shared is True and plain.seed_shared is False
	for trace in (False, True):
		a, b = seeded.search(qids, K_TOP, K_STEP, n_rounds, trace=trace), plain.search(qids, K_TOP, K_STEP, n_rounds, trace=trace)
		torch.cuda.synchronize()
		assert torch.equal(_bits(a.values), _bits(b.values)) and torch.equal(a.indices, b.indices)
		assert a.n_fallback == b.n_fallback and a.n_scored == b.n_scored == kc + n_rounds * K_STEP
	rounds_a, rounds_b = a.trace[:-1], b.trace[:-1]
	assert len(rounds_a) == len(rounds_b) == n_rounds - 1
	for r, (ta, tb) in enumerate(zip(rounds_a, rounds_b), start=2):
		assert (ta["order_ids"][:, :kc].cpu().numpy() == anc[None, :]).all()          # the rows begin with the anchors in the index' order
		for key in ("order_ids", "order_scores", "status", "W"):
			assert torch.equal(_bits(ta[key]), _bits(tb[key])), (r, key)
		# and the round is what lstsq_rows returns on the rows it was given
		W_ref, status_ref = ops.lstsq_rows(index.adaptive_operand()._Et, ta["order_ids"], ta["order_scores"], 0.0)
		ok = status_ref == 0
		assert torch.equal(ta["status"], status_ref) and torch.equal(_bits(ta["W"])[ok], _bits(W_ref)[ok]), r


def test_rank_deficient_query_falls_back_the_same_way(ops):
	"""Two identical Rt rows among query 0's first candidates: its solve fails from round 2 on, seeded or not, and the host row is the same."""
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, anc = _setup(24)
	R, _ = _matrices()
	qids = torch.arange(Q, dtype=torch.int64)
	X = scorer(qids, ops.as_index(anc, R.device, M))
	a, b = (int(x) for x in index.topk(X, K_STEP, exclude=ops.exclusion(anc, 0, M, R.device)).indices[0, :2].cpu().numpy())
	R2 = R.clone()
	R2[:, b] = R2[:, a]                                            # item b scores as item a does under every anchor query
	index2 = CURRowIndex(R2, anc, compute_dtype="fp32", pinv_backend="numpy")
	res = [AdaptiveSearcher(index2, scorer, incremental=True, seed_shared=s).search(qids, K_TOP, K_STEP, 3, trace=True) for s in (True, False)]
	torch.cuda.synchronize()
	first = res[0].trace[0]["order_ids"][0].cpu().numpy()
	assert a in first and b in first                               # (the premise: both are among query 0's first candidates)
	assert res[0].n_fallback == res[1].n_fallback >= 1
	assert torch.equal(_bits(res[0].values), _bits(res[1].values)) and torch.equal(res[0].indices, res[1].indices)
	for ta, tb in zip(res[0].trace[:-1], res[1].trace[:-1]):
		assert ta["status"][0].item() == 1 and torch.equal(ta["status"], tb["status"]) and torch.equal(_bits(ta["W"]), _bits(tb["W"]))
