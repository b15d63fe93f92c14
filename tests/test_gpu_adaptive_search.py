"""anncur_amd.search.AdaptiveSearcher end to end, on the three routes, from its trace.

Data: A = U V / sqrt(12) + noise N (rank-12 structure plus noise), the first kq rows are the anchor queries R, the next Q = 48 the test
queries the MatrixScorer answers from.  The two shapes put the per-query solve on either side:
  fp32 dense        m = 6000, kq = 256, kc = 24, k_step = 12, 4 rounds: n = 36, 48, 60 <= kq    (item side)
  bf16 and bf16x3   m = 8475, kq = 16,  kc = 32, k_step = 16, 3 rounds: n = 48, 64 > kq         (query side)
m = 8475 = 8448 + a ragged 27 lies just above the 8320 items from which ops.fused_supported takes retrievals of this size (k_step plus the
excluded S_q, at Kp = 64); the tests assert the route.  The noise levels (0.4 / 0.3) were chosen with an fp64 numpy simulation of the rounds
so that cond_2(R[:, S_q]) stays under 32 (largest seen: 28 / 18); the test recomputes cond_2 from the traced ids on the host and holds the
share of rows over 32 to 10 %.  The bound on W is that of tests/test_gpu_lstsq_rows.py.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, K_TOP, RANK = 48, 10, 12
CASES = {
	"fp32": dict(m=6000, kq=256, kc=24, k_step=12, n_rounds=4, noise=0.4, seed=1),
	"bf16": dict(m=8475, kq=16, kc=32, k_step=16, n_rounds=3, noise=0.3, seed=2),
	"bf16x3": dict(m=8475, kq=16, kc=32, k_step=16, n_rounds=3, noise=0.3, seed=2),
}


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=None)
def _data(m, kq, noise, seed):
	rng = np.random.default_rng(seed)
	U, V = rng.standard_normal((kq + Q, RANK)), rng.standard_normal((RANK, m))
	A = (U @ V / np.sqrt(RANK) + noise * rng.standard_normal((kq + Q, m))).astype(np.float32)
	return A[:kq].copy(), A[kq:].copy()


@functools.lru_cache(maxsize=None)
def _setup(dtype):
	"""(index, scorer, A_test on the host as the scorer sees it, Rt fp64 on the host as the solve sees it, anchors, case)."""
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import MatrixScorer
	c = CASES[dtype]
	R, At = _data(c["m"], c["kq"], c["noise"], c["seed"])
	anc = np.sort(np.random.default_rng(c["seed"] + 1).choice(c["m"], c["kc"], replace=False))
	Rd = torch.from_numpy(R).cuda()
	if dtype == "bf16":
		Rd = Rd.bfloat16()
	index = CURRowIndex(Rd, anc, compute_dtype=dtype, pinv_backend="numpy")
	A = torch.from_numpy(At).cuda()
	return index, MatrixScorer(A), At, Rd.float().cpu().numpy().astype(np.float64).T.copy(), anc, c


@functools.lru_cache(maxsize=None)
def _run(dtype):
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, Rt, anc, c = _setup(dtype)
	qids = torch.arange(Q, dtype=torch.int64)
	res = AdaptiveSearcher(index, scorer).search(qids, K_TOP, c["k_step"], c["n_rounds"], trace=True)
	torch.cuda.synchronize()
	return res


def _direct(ops, dtype, operand, W, excl, k_step, n_excl):
	"""The round's retrieval as a direct call of the route's ops."""
	m = operand.m
	if dtype == "fp32":
		assert operand._Etp is None and operand._split is None
		return ops.filter_topk(*ops.score_topk_dense(W, operand._Et, k_step + n_excl), excl, k_step)
	if dtype == "bf16":
		Kp = operand._Etp.shape[1]
		assert ops.fused_supported(Q, m, Kp, k_step + n_excl)
		return ops.filter_topk(*ops.score_topk_fused(ops.pack_bf16(W, Kp), operand._Etp_sorted, m, k_step + n_excl, leading_sample=True, item_ids=operand._item_ids), excl, k_step)
	assert ops.fused_supported(Q, m, operand._split.kp, ops.split_candidates(m, k_step, n_excl=n_excl))
	return ops.score_topk_split(W, operand._Et, operand._split.sorted, m, k_step, item_ids=operand._split.item_ids, leading_sample=True, exclude=excl)


def _topk_numpy(ids, scores, k):
	"""Rows of (ids, scores) -> the k best by score descending, ties to the smaller id."""
	out_v, out_i = np.empty((ids.shape[0], k), np.float32), np.empty((ids.shape[0], k), np.int32)
	for q in range(ids.shape[0]):
		order = np.lexsort((ids[q], -scores[q].astype(np.float64)))[:k]
		out_v[q], out_i[q] = scores[q][order], ids[q][order]
	return out_v, out_i


@pytest.mark.parametrize("dtype", list(CASES))
def test_one_round_is_cross_encoder_searcher(ops, dtype):
	from anncur_amd.search import AdaptiveSearcher, CrossEncoderSearcher
	index, scorer, At, Rt, anc, c = _setup(dtype)
	qids = torch.arange(Q, dtype=torch.int64)
	k_retvr = c["k_step"] * c["n_rounds"]
	want = CrossEncoderSearcher(index, scorer).search(qids, K_TOP, k_retvr)
	got = AdaptiveSearcher(index, scorer).search(qids, K_TOP, k_retvr, 1)
	assert torch.equal(got.values.view(torch.int32), want.values.view(torch.int32)) and torch.equal(got.indices, want.indices)
	assert got.n_scored == want.n_scored == c["kc"] + k_retvr and got.n_fallback == 0


@pytest.mark.parametrize("dtype", list(CASES))
def test_rounds_from_trace(ops, dtype):
	index, scorer, At, Rt, anc, c = _setup(dtype)
	res = _run(dtype)
	operand = index.adaptive_operand()
	rounds, final = res.trace[:-1], res.trace[-1]
	assert len(rounds) == c["n_rounds"] - 1
	over = total = 0
	for r, t in enumerate(rounds, start=2):
		ids, sc = t["ids"].cpu().numpy(), t["scores"].cpu().numpy()
		W, status = t["W"].cpu().numpy(), t["status"].cpu().numpy()
		n = c["kc"] + (r - 1) * c["k_step"]
		assert ids.shape == (Q, n) and (np.diff(ids.astype(np.int64), axis=1) > 0).all() and ids.min() >= 0   # strictly ascending: nothing scored twice
		assert all(np.isin(anc, row).all() for row in ids)
		assert np.array_equal(sc, At[np.arange(Q)[:, None], ids])
		assert not status.any() and np.isfinite(W).all()
		worst = 0.0
		for q in range(Q):
			Rs = Rt[ids[q]].T                                       # kq x n, the fp32 values the solve read
			U, s, Vt = np.linalg.svd(Rs, full_matrices=False)
			total += 1
			if s[0] / s[-1] > 32:
				over += 1
				continue
			w = ((sc[q].astype(np.float64) @ Vt.T) / s) @ U.T
			err, bound = np.abs(W[q] - w), 2.0 ** -24 * np.abs(w) + 2.0 ** -30 * np.linalg.norm(w)
			worst = max(worst, float((err / bound).max()))
			assert (err <= bound).all(), (dtype, r, q, float((err / bound).max()))
		print(f"{dtype} round {r}: n = {n}, worst err / bound = {worst:.3f}, rows over cond 32 so far: {over}")
		# the wiring: the same route, called directly on the traced W and the traced exclusion (normalised on the host)
		assert t["route"] == ("dense" if dtype == "fp32" else dtype)
		excl = ops.exclusion(ids, Q, c["m"], t["W"].device)
		want = _direct(ops, dtype, operand, t["W"], excl, c["k_step"], n)
		got = t["candidates"]
		assert torch.equal(got.indices, want.indices) and torch.equal(got.values.view(torch.int32), want.values.view(torch.int32))
		cand = got.indices.cpu().numpy()
		assert cand.min() >= 0 and not any(np.isin(cand[q], ids[q]).any() for q in range(Q))   # new items only: no anchor, nothing scored before
	assert over <= 0.1 * total, (over, total)
	# the end: the k best by exact score over the final S_q
	ids, sc = final["ids"].cpu().numpy(), final["scores"].cpu().numpy()
	assert ids.shape == (Q, c["kc"] + c["n_rounds"] * c["k_step"]) and (np.diff(ids.astype(np.int64), axis=1) > 0).all()
	assert np.array_equal(sc, At[np.arange(Q)[:, None], ids])
	want_v, want_i = _topk_numpy(ids, sc, K_TOP)
	assert np.array_equal(res.indices.cpu().numpy(), want_i) and np.array_equal(res.values.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
	assert res.n_scored == c["kc"] + c["n_rounds"] * c["k_step"] and res.n_fallback == 0


def test_rank_deficient_data_falls_back_to_the_host(ops):
	"""Exact integer rank 8 with kq = 16: every R[:, S_q] is singular, every solve reports status 1 and every query is solved by numpy."""
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	m, kq, kc, k_step, n_rounds = 3000, 16, 12, 10, 3
	rng = np.random.default_rng(8)
	A = (rng.integers(-3, 4, (kq + Q, 8)) @ rng.integers(-3, 4, (8, m))).astype(np.float32)
	assert np.linalg.matrix_rank(A.astype(np.float64)) == 8
	R, At = A[:kq], A[kq:]
	anc = np.sort(rng.choice(m, kc, replace=False))
	index = CURRowIndex(torch.from_numpy(R).cuda(), anc, compute_dtype="fp32", pinv_backend="numpy")
	res = AdaptiveSearcher(index, MatrixScorer(torch.from_numpy(At).cuda())).search(torch.arange(Q, dtype=torch.int64), K_TOP, k_step, n_rounds, trace=True)
	torch.cuda.synchronize()
	assert res.n_fallback == Q and res.n_scored == kc + n_rounds * k_step
	operand = index.adaptive_operand()
	for r, t in enumerate(res.trace[:-1], start=2):
		ids = t["ids"].cpu().numpy()
		assert (np.diff(ids.astype(np.int64), axis=1) > 0).all() and ids.min() >= 0
		assert (t["status"].cpu().numpy() == 1).all() and np.isfinite(t["W"].cpu().numpy()).all()
		excl = ops.exclusion(ids, Q, m, t["W"].device)
		want = _direct(ops, "fp32", operand, t["W"], excl, k_step, ids.shape[1])
		assert torch.equal(t["candidates"].indices, want.indices)
	ids, sc = res.trace[-1]["ids"].cpu().numpy(), res.trace[-1]["scores"].cpu().numpy()
	assert (np.diff(ids.astype(np.int64), axis=1) > 0).all() and np.array_equal(sc, At[np.arange(Q)[:, None], ids])
	want_v, want_i = _topk_numpy(ids, sc, K_TOP)
	assert np.array_equal(res.indices.cpu().numpy(), want_i) and np.array_equal(res.values.cpu().numpy(), want_v)


def test_recall_by_rounds_is_printed(ops):
	"""A record, not a gate: recall@10 of 1, 2 and 4 rounds at the budget kc + 48 on the fp32 case."""
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, Rt, anc, c = _setup("fp32")
	exact = np.argsort(-At, axis=1, kind="stable")[:, :K_TOP]
	for n_rounds in (1, 2, 4):
		res = AdaptiveSearcher(index, scorer).search(torch.arange(Q, dtype=torch.int64), K_TOP, 48 // n_rounds, n_rounds)
		got = res.indices.cpu().numpy()
		rec = np.mean([np.isin(exact[q], got[q]).mean() for q in range(Q)])
		print(f"recall@{K_TOP} at budget {c['kc']} + 48, n_rounds = {n_rounds}: {rec:.4f}")
		assert res.n_scored == c["kc"] + 48
