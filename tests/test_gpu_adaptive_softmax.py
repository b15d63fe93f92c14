"""AdaptiveSearcher(strategy="softmax") end to end, from its trace, in the small fp32 setting of tests/test_gpu_adaptive_search.py:
A = U V / sqrt(12) + 0.4 N, Q = 48 test queries, m = 6000 items, kq = 256 anchor queries, 24 anchor items, k_step = 12, MatrixScorer.

The strategy changes how a round picks its items, not what surrounds the pick: every round's candidates must be, bit for bit, the host
statement of the sampler (tests/gumbel_numpy.py) on that round's dense scores, the device's noise of (seed, stream = round, row key = query
id) and the traced exclusion; the default strategy stays today's search; and entry point B reports the sampled search under its own
prefix.  Needs an MI355X."""
import functools
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_numpy as gn  # noqa: E402

pytestmark = pytest.mark.gpu

Q, K_TOP, RANK = 48, 10, 12
M, KQ, KC, K_STEP, N_ROUNDS, NOISE, SEED = 6000, 256, 24, 12, 4, 0.4, 1
TEMP, NOISE_SEED = 0.5, 2024


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


@functools.lru_cache(maxsize=None)
def _setup():
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import MatrixScorer
	R, At, anc = _data()
	index = CURRowIndex(torch.from_numpy(R).cuda(), anc, compute_dtype="fp32", pinv_backend="numpy")
	return index, MatrixScorer(torch.from_numpy(At).cuda()), At, anc


def _qids():
	return torch.arange(Q, dtype=torch.int64)


def _soft(incremental=False, seed=NOISE_SEED, **kw):
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, _, _ = _setup()
	return AdaptiveSearcher(index, scorer, incremental=incremental, strategy="softmax", temperature=TEMP, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def _run(incremental):
	res = _soft(incremental).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
	torch.cuda.synchronize()
	return res


def _same(a, b):
	return torch.equal(a.indices, b.indices) and torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))


def test_default_strategy_is_the_search_as_it_was(ops):
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, _, _ = _setup()
	for incremental in (False, True):
		old = AdaptiveSearcher(index, scorer, incremental=incremental).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
		new = AdaptiveSearcher(index, scorer, incremental=incremental, strategy="topk", temperature=0.3, seed=99).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
		assert _same(old, new) and old.n_scored == new.n_scored and old.n_fallback == new.n_fallback
		for a, b in zip(old.trace[:-1], new.trace[:-1]):
			assert _same(a["candidates"], b["candidates"]) and a["route"] == b["route"] == "dense"
			assert torch.equal(a["W"].view(torch.int32), b["W"].view(torch.int32)) and torch.equal(a["ids"], b["ids"])


def _reference_round(ops, scores_dev, r, excluded, qids=None):
	"""Round r's draw on the host: the dense scores, the device's noise of (seed, stream r, the query ids), the excluded ids per query."""
	G = ops.gumbel_noise(NOISE_SEED, r, _qids() if qids is None else qids, M).cpu().numpy()
	return gn.sample_reference(scores_dev.cpu().numpy(), np.float32(1.0 / TEMP), G, K_STEP, excluded)


@pytest.mark.parametrize("incremental", [False, True])
def test_every_round_is_the_host_statement_of_the_draw(ops, incremental):
	index, scorer, At, anc = _setup()
	res = _run(incremental)
	Rt = index.adaptive_operand()._Et
	rounds, final = res.trace[:-1], res.trace[-1]
	assert len(rounds) == N_ROUNDS - 1 and res.n_scored == KC + N_ROUNDS * K_STEP and res.n_fallback == 0
	# round 1 leaves no trace entry of its own: its candidates are what round 2's S_q holds beyond the anchors
	X = scorer(_qids(), ops.as_index(anc, index.R.device, M))
	want_v, want_i = _reference_round(ops, ops.gemm(X, index._Et.t()), 1, [anc] * Q)
	ids2 = rounds[0]["ids"].cpu().numpy()
	assert all(np.array_equal(np.setdiff1d(ids2[q], anc), np.sort(want_i[q])) for q in range(Q))
	if incremental:
		assert np.array_equal(rounds[0]["order_ids"].cpu().numpy()[:, KC:], want_i)                      # ... in the order they were drawn
	direct = index.sample(X, K_STEP, TEMP, NOISE_SEED, 1, _qids(), ops.exclusion(anc, 0, M, index.R.device))
	assert np.array_equal(direct.indices.cpu().numpy(), want_i) and np.array_equal(direct.values.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
	for r, t in enumerate(rounds, start=2):
		ids, sc = t["ids"].cpu().numpy(), t["scores"].cpu().numpy()
		n = KC + (r - 1) * K_STEP
		assert ids.shape == (Q, n) and (np.diff(ids.astype(np.int64), axis=1) > 0).all() and ids.min() >= 0    # strictly ascending: nothing scored twice
		assert all(np.isin(anc, row).all() for row in ids) and np.array_equal(sc, At[np.arange(Q)[:, None], ids])
		assert t["route"] == "sample-dense" and not t["status"].any().item()
		want_v, want_i = _reference_round(ops, ops.gemm(t["W"], Rt.t()), r, ids)
		got = t["candidates"]
		assert np.array_equal(got.indices.cpu().numpy(), want_i), r
		assert np.array_equal(got.values.cpu().numpy().view(np.uint32), want_v.view(np.uint32)), r
		cand = want_i
		assert cand.min() >= 0 and all(np.unique(cand[q]).size == K_STEP for q in range(Q))                    # distinct ...
		assert not any(np.isin(cand[q], ids[q]).any() for q in range(Q))                                       # ... and disjoint from S_q
		if incremental:    # W is lstsq_rows on the rows in insertion order, as for the default strategy
			W_ref, _ = ops.lstsq_rows(Rt, t["order_ids"], t["order_scores"], 0.0)
			assert torch.equal(t["W"].view(torch.int32), W_ref.view(torch.int32))
			assert np.array_equal(np.sort(t["order_ids"].cpu().numpy(), axis=1), ids)
	# the end: the k best by exact score over everything scored
	ids, sc = final["ids"], final["scores"]
	assert tuple(ids.shape) == (Q, KC + N_ROUNDS * K_STEP) and np.array_equal(sc.cpu().numpy(), At[np.arange(Q)[:, None], ids.cpu().numpy()])
	assert _same(res, ops.rerank_scored(K_TOP, ids, sc))


def test_seed_and_row_keys(ops):
	res = _run(False)
	again = _soft().search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
	assert _same(res, again) and all(_same(a["candidates"], b["candidates"]) for a, b in zip(res.trace[:-1], again.trace[:-1]))     # the same seed: the same search
	other = _soft(seed=NOISE_SEED + 1).search(_qids(), K_TOP, K_STEP, N_ROUNDS, trace=True)
	assert other.n_scored == res.n_scored
	assert not torch.equal(other.trace[0]["candidates"].indices, res.trace[0]["candidates"].indices)                              # another seed: another draw
	assert not torch.equal(other.trace[-1]["ids"], res.trace[-1]["ids"])
	# the row-key contract: a query draws the same items wherever it stands in query_ids
	perm = torch.from_numpy(np.random.default_rng(4).permutation(Q))
	moved = _soft().search(perm, K_TOP, K_STEP, N_ROUNDS, trace=True)
	pd = perm.cuda()
	assert torch.equal(moved.indices, res.indices[pd]) and torch.equal(moved.values.view(torch.int32), res.values[pd].view(torch.int32))
	for a, b in zip(moved.trace[:-1], res.trace[:-1]):
		assert torch.equal(a["candidates"].indices, b["candidates"].indices[pd])
	assert torch.equal(moved.trace[-1]["ids"], res.trace[-1]["ids"][pd])


def test_one_sampled_round(ops):
	"""n_rounds = 1 with softmax: one sampled round, then the re-rank over anchors + the drawn items."""
	index, scorer, At, anc = _setup()
	k_retvr = K_STEP * N_ROUNDS
	res = _soft().search(_qids(), K_TOP, k_retvr, 1, trace=True)
	assert res.trace == [] and res.n_scored == KC + k_retvr and res.n_fallback == 0
	X = scorer(_qids(), ops.as_index(anc, index.R.device, M))
	cand = index.sample(X, k_retvr, TEMP, NOISE_SEED, 1, _qids(), anc)
	want = ops.rerank_scored(K_TOP, cand.indices, scorer(_qids(), cand.indices), ops.shared_id_list(anc, index.R.device), X)
	assert _same(res, want)


def test_recall_by_rounds_and_strategy_is_printed(ops):
	"""A record, not a gate: recall@10 of 1, 2 and 4 rounds at the budget kc + 48, both strategies."""
	from anncur_amd.search import AdaptiveSearcher
	index, scorer, At, anc = _setup()
	exact = np.argsort(-At, axis=1, kind="stable")[:, :K_TOP]
	for name, kw in (("topk", {}), (f"softmax T = {TEMP}", dict(strategy="softmax", temperature=TEMP, seed=NOISE_SEED)),
					 ("softmax T = 0.1", dict(strategy="softmax", temperature=0.1, seed=NOISE_SEED))):
		for n_rounds in (1, 2, 4):
			res = AdaptiveSearcher(index, scorer, **kw).search(_qids(), K_TOP, 48 // n_rounds, n_rounds)
			got = res.indices.cpu().numpy()
			rec = np.mean([np.isin(exact[q], got[q]).mean() for q in range(Q)])
			print(f"recall@{K_TOP} at budget {KC} + 48, {name}, n_rounds = {n_rounds}: {rec:.4f}")
			assert res.n_scored == KC + 48


# ------------------------------------------------------------------ entry point B
OLD, TOPK, SOFT = "exact_vs_reranked_approx_retvr", "exact_vs_reranked_adaptive_retvr", "exact_vs_reranked_adaptive_softmax_retvr"


def _dump(path, scores, **extra):
	os.makedirs(os.path.dirname(path), exist_ok=True)
	d = {"ment_to_ent_scores": scores, "ment_to_ent_scores.shape": tuple(scores.shape), "test_data": [], "mention_tokens_list": [[0] * 4] * scores.shape[0],
		 "entity_id_list": np.arange(scores.shape[1]), "entity_tokens_list": [], "arg_dict": {}}
	d.update(extra)
	with open(path, "wb") as f:
		pickle.dump(d, f)


def _stats(counts, n, prefix):
	"""The reference's statistics of per-query overlap counts, restated: np.mean / population np.std / np.percentile 50, 4 decimals."""
	c = np.asarray(counts, dtype=np.float64)
	out = {}
	for metric, v in (("common", c), ("diff", n - c), ("total", np.full_like(c, n)), ("common_frac", c / n), ("diff_frac", (n - c) / n)):
		for name, x in (("mean", np.mean(v)), ("std", np.std(v)), ("p50", np.percentile(v, 50))):
			out[f"{prefix}~{metric}_{name}"] = float("{:.4f}".format(x))
	return out


def test_entry_point_B_softmax_metrics(ops, tmp_path):
	"""The synthetic pickles of tests/test_gpu_entrypoint_adaptive.py (built here the same way).  --adaptive_strategy softmax with N = 2: the
	new prefix, with the usual nesting, holds the closed form |exact[:k] & pool| of a direct sampled search; every other metric is the run's
	without the flags; the flags at their defaults write what no flag writes."""
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	top_k, retr, ancs = [1, 10], [5, 10, 50], [10, 20]
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			  "--train_data_file", str(tmp_path / "train.pkl"), "--top_k_vals", "1,10", "--top_k_retr_vals", "5,10,50", "--n_ent_anchors_vals", "10,20", "--pinv", "numpy"]
	f_old = epB.main(common + ["--misc", "old"])
	f_dflt = epB.main(common + ["--misc", "dflt", "--adaptive_strategy", "topk", "--adaptive_temperature", "1.0", "--adaptive_seed", "0"])
	f_lone = epB.main(common + ["--misc", "lone", "--adaptive_strategy", "softmax"])                  # without --adaptive_rounds N >= 2: no effect on the metrics
	f_topk = epB.main(common + ["--misc", "topk", "--adaptive_rounds", "2"])
	f_soft = epB.main(common + ["--misc", "soft", "--adaptive_rounds", "2", "--adaptive_strategy", "softmax", "--adaptive_temperature", "0.25", "--adaptive_seed", "5"])
	assert open(f_dflt).read().replace('"misc": "dflt"', '"misc": "old"') == open(f_old).read()       # the defaults write what no flag writes
	old, lone, topk, soft = (json.load(open(f)) for f in (f_old, f_lone, f_topk, f_soft))
	assert {k: v for k, v in lone.items() if k != "other_args"} == {k: v for k, v in old.items() if k != "other_args"} and lone["other_args"]["adaptive_strategy"] == "softmax"
	assert not any(key in topk["other_args"] for key in ("adaptive_strategy", "adaptive_temperature", "adaptive_seed"))
	assert [soft["other_args"][key] for key in ("adaptive_rounds", "adaptive_strategy", "adaptive_temperature", "adaptive_seed")] == [2, "softmax", 0.25, 5]
	At_dev, Atr_dev = A_test.cuda(), A_train.cuda()
	qids = torch.arange(40, dtype=torch.int64)
	rng = np.random.default_rng(0)
	n_cells = 0
	for n_anc in ancs:
		anc = sorted(rng.choice(600, size=n_anc, replace=False))
		searcher = AdaptiveSearcher(CURRowIndex(Atr_dev, np.asarray(anc), compute_dtype=None, pinv_backend="numpy"), MatrixScorer(At_dev), strategy="softmax",
									temperature=0.25, seed=5)
		for kr in retr:
			pool = searcher.search(qids, 1, kr // 2, 2, trace=True).trace[-1]["ids"].cpu().numpy() if kr % 2 == 0 else None
			for k in top_k:
				if k > kr:
					continue
				where = (f"top_k={k}", f"k_retvr={kr}", f"anc_n_m=60_anc_n_e={n_anc}")
				o, t, s = (d["seed=0"][where[0]][where[1]][where[2]] for d in (old, topk, soft))
				assert {m: v for m, v in s.items() if not m.startswith(SOFT + "~")} == o                                 # every old metric: equal
				assert not any(m.startswith(TOPK + "~") for m in s) and not any(m.startswith(SOFT + "~") for m in t)     # each strategy under its own prefix
				new_keys = {m for m in s if m.startswith(SOFT + "~")}
				if pool is None:
					assert not new_keys
					continue
				assert {m[len(SOFT):] for m in new_keys} == {m[len(TOPK):] for m in t if m.startswith(TOPK + "~")}       # the usual nesting: the same statistics
				assert pool.shape == (40, n_anc + kr) and all(np.isin(anc, row).all() for row in pool)
				counts = [len(set(torch.topk(A_test[q], k).indices.tolist()) & set(pool[q].tolist())) for q in range(40)]
				assert {m: s[m] for m in new_keys} == _stats(counts, k, SOFT), (k, kr, n_anc)
				n_cells += 1
	assert n_cells == 2 * (2 + 2)          # per anchor count: k_retvr 10 and 50, two top_k each; k_retvr 5 is odd
