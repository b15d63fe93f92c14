"""AdaptiveSearcher(incremental=True) end to end, from its trace, in the small fp32 setting of tests/test_gpu_adaptive_search.py:
A = U V / sqrt(12) + 0.4 N, Q = 48 test queries, m = 6000 items, kq = 256 anchor queries, 24 anchor items, k_step = 12, MatrixScorer.

The switch changes how the weights of a round are computed, not what they are: every round's W must be, bit for bit, ops.lstsq_rows on
the rows in insertion order that the trace records ("order_ids" / "order_scores"); everything around the solve -- the exclusion from the
id-sorted copy, the scorer never asked twice, the final re-rank -- is checked as for the default searcher.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, K_TOP, RANK = 48, 10, 12
M, KQ, KC, K_STEP, N_ROUNDS, NOISE, SEED = 6000, 256, 24, 12, 4, 0.4, 1


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=None)
def _data():
	rng = np.random.default_rng(SEED)
	U, V = rng.standard_normal((KQ + Q, RANK)), rng.standard_normal((RANK, M))
	A = (U @ V / np.sqrt(RANK) + NOISE * rng.standard_normal((KQ + Q, M))).astype(np.float32)
	anc = np.sort(np.random.default_rng(SEED + 1).choice(M, KC, replace=False))
	return A[:KQ].copy(), A[KQ:].copy(), anc


def _index(R, anc):
	from anncur_amd.cur import CURRowIndex
	return CURRowIndex(torch.from_numpy(R).cuda(), anc, compute_dtype="fp32", pinv_backend="numpy")


@functools.lru_cache(maxsize=None)
def _setup():
	from anncur_amd.search import MatrixScorer
	R, At, anc = _data()
	return _index(R, anc), MatrixScorer(torch.from_numpy(At).cuda()), At, anc


def _qids():
	return torch.arange(Q, dtype=torch.int64)


def _check_rounds(ops, res, index, At, anc, expect_failed):
	"""The trace of an incremental run: per round the solve's rows, W against lstsq_rows, the wiring around it; expect_failed(order_ids) ->
	the bool [Q] of queries whose solve must report status 1.  -> the set of queries that failed in any round."""
	Rt = index.adaptive_operand()._Et
	rounds, final = res.trace[:-1], res.trace[-1]
	assert len(rounds) == N_ROUNDS - 1
	failed_any = set()
	for r, t in enumerate(rounds, start=2):
		n = KC + (r - 1) * K_STEP
		o_ids, o_sc = t["order_ids"], t["order_scores"]
		assert tuple(o_ids.shape) == (Q, n) and tuple(o_sc.shape) == (Q, n)
		oi, osc, ids, sc = o_ids.cpu().numpy(), o_sc.cpu().numpy(), t["ids"].cpu().numpy(), t["scores"].cpu().numpy()
		# insertion order: the anchors in the index' order, then every earlier round's candidates in retrieval order
		assert (oi[:, :KC] == anc[None, :]).all()
		assert np.array_equal(oi[:, KC:KC + K_STEP], first_candidates(index).cpu().numpy()) if r == 2 else np.array_equal(oi[:, :n - K_STEP], prev_oi)
		if r > 2:
			assert np.array_equal(oi[:, n - K_STEP:], prev_cand)
		# the same set as the id-sorted copy, which is strictly ascending: nothing scored twice
		assert (np.diff(ids.astype(np.int64), axis=1) > 0).all() and ids.min() >= 0 and np.array_equal(np.sort(oi, axis=1), ids)
		assert np.array_equal(osc, At[np.arange(Q)[:, None], oi]) and np.array_equal(sc, At[np.arange(Q)[:, None], ids])
		# W: bit for bit lstsq_rows on the ordered rows; a failed query holds the host's finite row instead of NaN
		W_ref, status_ref = ops.lstsq_rows(Rt, o_ids, o_sc, 0.0)
		W, status, W_ref, status_ref = t["W"].cpu().numpy(), t["status"].cpu().numpy(), W_ref.cpu().numpy(), status_ref.cpu().numpy()
		want_failed = expect_failed(oi)
		assert np.array_equal(status, status_ref) and np.array_equal(status != 0, want_failed), (r, np.nonzero(status)[0], np.nonzero(want_failed)[0])
		ok = ~want_failed
		assert np.array_equal(W[ok].view(np.uint32), W_ref[ok].view(np.uint32)), r
		assert np.isfinite(W).all() and np.isnan(W_ref[want_failed]).all()
		failed_any.update(np.nonzero(want_failed)[0].tolist())
		cand = t["candidates"].indices.cpu().numpy()
		assert cand.min() >= 0 and not any(np.isin(cand[q], ids[q]).any() for q in range(Q))   # new items only
		prev_oi, prev_cand = oi, cand
	# the end: n_scored, and the k best by exact score over everything scored
	ids, sc = final["ids"], final["scores"]
	ids_h = ids.cpu().numpy()
	assert res.n_scored == KC + N_ROUNDS * K_STEP == ids_h.shape[1] and (np.diff(ids_h.astype(np.int64), axis=1) > 0).all()
	assert np.array_equal(sc.cpu().numpy(), At[np.arange(Q)[:, None], ids_h])
	want = ops.rerank_scored(K_TOP, ids, sc)
	assert torch.equal(res.indices, want.indices) and torch.equal(res.values.view(torch.int32), want.values.view(torch.int32))
	return failed_any


def first_candidates(index):
	"""Round 1 as a direct call: the k_step best of the index outside the anchors."""
	from anncur_amd import ops
	_, scorer, _, anc = _setup()
	X = scorer(_qids(), ops.as_index(anc, index.R.device, M))
	return index.topk(X, K_STEP, exclude=ops.exclusion(anc, 0, M, index.R.device)).indices


def test_rounds_are_lstsq_rows_on_the_insertion_order(ops):
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, anc = _setup()
	res = AdaptiveSearcher(index, scorer, incremental=True).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
	torch.cuda.synchronize()
	failed = _check_rounds(ops, res, index, At, anc, lambda oi: np.zeros(Q, dtype=bool))
	assert not failed and res.n_fallback == 0


def test_one_round_with_the_switch_is_cross_encoder_searcher(ops):
	from anncur_amd.search import AdaptiveSearcher, CrossEncoderSearcher
	index, scorer, At, anc = _setup()
	k_retvr = K_STEP * N_ROUNDS
	want = CrossEncoderSearcher(index, scorer).search(_qids(), K_TOP, k_retvr)
	got = AdaptiveSearcher(index, scorer, incremental=True).search(_qids(), K_TOP, k_retvr, 1, trace=True)
	assert torch.equal(got.values.view(torch.int32), want.values.view(torch.int32)) and torch.equal(got.indices, want.indices)
	assert got.n_scored == want.n_scored == KC + k_retvr and got.n_fallback == 0 and got.trace == []


def test_rank_deficient_query_takes_the_host_fallback_in_every_later_round(ops):
	"""Two identical Rt rows among query 0's first candidates: from round 2 on its solve fails (the state's status is sticky), the host
	solves it every round and it is counted once.  Any other query that has scored both items fails the same way, from that round on."""
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, anc = _setup()
	a, b = (int(x) for x in first_candidates(index)[0, :2].cpu().numpy())
	R, _, _ = _data()
	R2 = R.copy()
	R2[:, b] = R2[:, a]                                            # item b scores as item a does under every anchor query
	index2 = _index(R2, anc)
	first = first_candidates(index2)[0].cpu().numpy()
	assert a in first and b in first                               # (the premise: both are still among query 0's first candidates)
	res = AdaptiveSearcher(index2, scorer, incremental=True).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
	torch.cuda.synchronize()
	failed = _check_rounds(ops, res, index2, At, anc, lambda oi: (oi == a).any(axis=1) & (oi == b).any(axis=1))
	assert 0 in failed and res.n_fallback == len(failed)
	assert all(t["status"][0].item() == 1 for t in res.trace[:-1])   # query 0: every round r >= 2


def test_recall_with_and_without_the_switch_is_printed(ops):
	"""A record, not a gate: the two paths factor the same matrix in different orders, so near-ties of a retrieval may fall differently."""
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, anc = _setup()
	exact = np.argsort(-At, axis=1, kind="stable")[:, :K_TOP]
	for incremental in (False, True):
		res = AdaptiveSearcher(index, scorer, incremental=incremental).search(_qids(), K_TOP, K_STEP, N_ROUNDS)
		got = res.indices.cpu().numpy()
		rec = np.mean([np.isin(exact[q], got[q]).mean() for q in range(Q)])
		print(f"recall@{K_TOP} at budget {KC} + {N_ROUNDS * K_STEP}, n_rounds = {N_ROUNDS}, incremental = {incremental}: {rec:.4f}")
		assert res.n_scored == KC + N_ROUNDS * K_STEP
