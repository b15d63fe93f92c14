"""--rerank_pool retrieved+anchors through both command-line entry points, on the small synthetic pickles of
tests/test_gpu_entrypoints.py (built here the same way): random low-rank fp32 scores, tie-free.

With the flag every CUR cell also reports, under exact_vs_reranked_approx_retvr_w_anchors~..., the overlap metrics of the pool "anchor
items + k_retvr NEW items".  Checked: the old prefix is untouched by the flag; the new prefix never loses against the old one at the same
cell (a superset pool cannot lose an exact top-k item); the new prefix equals a torch loop on the CPU written here (U from the same
numpy.linalg.pinv call, the products in float64); the literal re-rank (ops.rerank_scored on MatrixScorer scores) equals the closed
form; a cell over the limit shows under the old prefix only.  Needs an MI355X."""
import json
import logging
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OLD, NEW = "exact_vs_reranked_approx_retvr", "exact_vs_reranked_approx_retvr_w_anchors"


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


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


def _pool_counts(A, S_hat, anc, k, k_retvr):
	"""Per query |exact top-k of A  &  (anchors + the k_retvr best non-anchor items by S_hat)| in a torch loop on the CPU."""
	anc_t = torch.as_tensor(np.asarray(anc, dtype=np.int64))
	counts = []
	for q in range(A.shape[0]):
		s = S_hat[q].clone()
		s[anc_t] = -float("inf")
		pool = set(anc_t.tolist()) | set(torch.topk(s, k_retvr).indices.tolist())
		counts.append(len(pool & set(torch.topk(A[q], k).indices.tolist())))
	return np.asarray(counts)


def _entry_A_matrix():
	torch.manual_seed(0)
	return torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)


def test_entry_point_A_pool_metrics(gpu, tmp_path, caplog):
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from utils.zeshel_utils import score_matrix_filename
	A = _entry_A_matrix()
	res_dir = str(tmp_path / "res")
	_dump(score_matrix_filename(res_dir, "yugioh", 1000), A)
	common = ["--data_name", "yugioh", "--res_dir", res_dir, "--n_ment", "1000", "--n_seeds", "2", "--disable_wandb", "1", "--eval_methods", "cur,cur_oracle",
			  "--n_ment_anchors_vals", "128", "--n_ent_anchors_vals", "64,2000", "--top_k_vals", "10", "--top_k_retr_vals", "100", "--pinv", "numpy"]
	out_old = epA.main(common + ["--misc", "old"])
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		out_new = epA.main(common + ["--misc", "new", "--rerank_pool", "retrieved+anchors"])
	old = json.load(open(os.path.join(out_old, "retrieval_wrt_exact_crossenc.json")))
	new = json.load(open(os.path.join(out_new, "retrieval_wrt_exact_crossenc.json")))
	assert "rerank_pool" not in old["other_args"]["arg_dict"] and new["other_args"]["arg_dict"]["rerank_pool"] == "retrieved+anchors"
	for method in ("cur", "cur_oracle"):
		for ne in (64, 2000):
			o = old[method]["top_k=10"]["k_retvr=100"][f"anc_n_m=128~anc_n_e={ne}"]
			n = new[method]["top_k=10"]["k_retvr=100"][f"anc_n_m=128~anc_n_e={ne}"]
			for t in ("anchor", "non_anchor", "all"):
				assert not any(m.startswith(NEW) for m in o[t])
				for m, v in o[t].items():   # the old prefix and the error norms: untouched by the flag
					assert n[t][m] == (pytest.approx(v, rel=1e-5) if m.startswith("approx_error") else v), (method, ne, t, m)
				new_keys = {m for m in n[t] if m.startswith(NEW + "~")}
				if ne == 2000:   # 100 + 2000 > min(5000, 2048): under the old prefix only
					assert not new_keys
					continue
				assert {m.replace(NEW, OLD) for m in new_keys} == {m for m in o[t] if m.startswith(OLD + "~")}
				assert n[t][f"{NEW}~common_mean"] >= o[t][f"{OLD}~common_mean"], (method, t)
	assert any("2048" in r.getMessage() and NEW in r.getMessage() for r in caplog.records), "the skipped cell is logged with the limit"
	# method cur against the CPU loop: anchors selected like the harness does, U from the same numpy call, float64 products
	want = {t: [] for t in ("anchor", "non_anchor", "all")}
	for seed in range(2):
		rng = np.random.default_rng(seed)
		ri = sorted(rng.choice(1000, 128, replace=False)); ci = sorted(rng.choice(5000, 64, replace=False))
		U = torch.from_numpy(np.linalg.pinv(A[ri][:, ci].numpy())).double()
		S_hat = A[:, ci].double() @ (U @ A[ri].double())
		counts = _pool_counts(A, S_hat, ci, 10, 100)
		non = sorted(set(range(1000)) - set(int(i) for i in ri))
		for t, rows in (("anchor", ri), ("non_anchor", non), ("all", list(range(1000)))):
			want[t].append(_stats(counts[np.asarray(rows, dtype=np.int64)], 10, NEW))
	cell = new["cur"]["top_k=10"]["k_retvr=100"]["anc_n_m=128~anc_n_e=64"]
	for t in want:
		for m in want[t][0]:
			assert cell[t][m] == float(np.mean([w[m] for w in want[t]])), (t, m, cell[t][m], [w[m] for w in want[t]])


def _entry_B_matrices():
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	return A_train, A_test


def test_entry_point_B_pool_metrics(gpu, tmp_path, caplog):
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	A_train, A_test = _entry_B_matrices()
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	top_k, retr, ancs = [1, 10, 50], [5, 10, 50, 580], [10, 20, 30]      # 580 + 30 > 600 items: one over-limit cell, at 30 anchors only
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			  "--train_data_file", str(tmp_path / "train.pkl"), "--n_seeds", "2", "--top_k_vals", "1,10,50", "--top_k_retr_vals", "5,10,50,580",
			  "--n_ent_anchors_vals", "10,20,30", "--pinv", "numpy"]
	f_old = epB.main(common + ["--misc", "old"])
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		f_new = epB.main(common + ["--misc", "new", "--rerank_pool", "retrieved+anchors"])
	old, new = json.load(open(f_old)), json.load(open(f_new))
	assert "rerank_pool" not in old["other_args"] and new["other_args"]["rerank_pool"] == "retrieved+anchors"
	n_cells = 0
	for seed in range(2):
		rng = np.random.default_rng(seed)                      # one stream over the anchor counts, as the harness (and the reference) draws
		for n_anc in ancs:
			anc = sorted(rng.choice(600, size=n_anc, replace=False))
			U = torch.from_numpy(np.linalg.pinv(A_train[:, anc].numpy())).double()
			S_hat = A_test[:, anc].double() @ (U @ A_train.double())
			for kr in retr:
				for k in top_k:
					if k > kr:
						assert f"k_retvr={kr}" not in new[f"seed={seed}"].get(f"top_k={k}", {})
						continue
					o = old[f"seed={seed}"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
					n = new[f"seed={seed}"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
					assert not any(m.startswith(NEW) for m in o)
					assert {m: v for m, v in n.items() if not m.startswith(NEW + "~")} == o            # every old-prefix metric: equal
					new_keys = {m for m in n if m.startswith(NEW + "~")}
					if kr + n_anc > 600:
						assert not new_keys, (k, kr, n_anc)                                            # the over-limit cell: old prefix only
						continue
					assert n[f"{NEW}~common_mean"] >= o[f"{OLD}~common_mean"], (seed, k, kr, n_anc)
					want = _stats(_pool_counts(A_test, S_hat, anc, k, kr), k, NEW)
					assert {m: n[m] for m in new_keys} == want, (seed, k, kr, n_anc)
					n_cells += 1
	assert n_cells == 2 * (3 * (1 + 2 + 3 + 3) - 3)                # per seed: 9 cells with top_k <= k_retvr per anchor count, less the 3 over the limit
	assert any("600" in r.getMessage() and NEW in r.getMessage() for r in caplog.records), "the skipped cell is logged with the limit"


def test_literal_rerank_equals_the_closed_form(gpu):
	"""harness level, both entry points: ops.rerank_scored on MatrixScorer scores per k_retvr against the one overlap call."""
	from anncur_amd import harness
	A_train, A_test = _entry_B_matrices()
	grids = {"top_k_vals": [1, 10, 50], "top_k_retr_vals": [5, 10, 50, 580], "n_ent_anchors_vals": [0, 10, 30]}
	for dtype in ("fp32", "bf16"):
		At, Aq = harness.to_device_matrix(A_train, "cuda", dtype), harness.to_device_matrix(A_test, "cuda", dtype)
		closed = harness.run_eval_method_cur(Aq, At, 1, grids, rerank_pool="retrieved+anchors", pinv_backend="numpy")
		literal = harness.run_eval_method_cur(Aq, At, 1, grids, rerank_pool="retrieved+anchors", pinv_backend="numpy", literal_rerank=True)
		assert closed == literal
		cell = closed["top_k=10"]["k_retvr=50"]
		assert f"{NEW}~common_mean" in cell["anc_n_m=60_anc_n_e=30"] and f"{NEW}~common_mean" in cell["anc_n_m=60_anc_n_e=0"]
		zero = closed["top_k=10"]["k_retvr=50"]["anc_n_m=60_anc_n_e=0"]                                # no anchors: the pool is the retrieved list
		assert all(zero[m.replace(OLD, NEW)] == v for m, v in zero.items() if m.startswith(OLD + "~"))
		plain = harness.run_eval_method_cur(Aq, At, 1, grids, pinv_backend="numpy")
		assert all(m.startswith(OLD + "~") for m in plain["top_k=10"]["k_retvr=50"]["anc_n_m=60_anc_n_e=30"])
	A = _entry_A_matrix().cuda()
	closed = harness.run_approx_eval_w_seed("cur", A, 128, 64, 10, 100, 0, pinv_backend="numpy", rerank_pool="retrieved+anchors")
	literal = harness.run_approx_eval_w_seed("cur", A, 128, 64, 10, 100, 0, pinv_backend="numpy", rerank_pool="retrieved+anchors", literal_rerank=True)
	for t in ("anchor", "non_anchor", "all"):
		assert {m: v for m, v in closed[t].items() if not m.startswith("approx_error")} == {m: v for m, v in literal[t].items() if not m.startswith("approx_error")}
		assert f"{NEW}~common_frac_mean" in closed[t]
	with pytest.raises(ValueError, match="rerank_pool"):
		harness.run_approx_eval_w_seed("cur", A, 128, 64, 10, 100, 0, rerank_pool="anchors")
