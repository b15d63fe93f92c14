"""--adaptive_rounds through entry point B, on the small synthetic pickles of tests/test_gpu_entrypoints_pool.py (built here the
same way): with N = 2 the new prefix is present for exactly the cells with even k_retvr inside the searcher's limits, every reported
statistic equals the closed form |exact[:k] & pool| recomputed here from a direct AdaptiveSearcher run, the cells left out are logged once
per anchor set, and N = 1 writes what no flag writes.  Needs an MI355X."""
import json
import logging
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OLD, NEW = "exact_vs_reranked_approx_retvr", "exact_vs_reranked_adaptive_retvr"


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


def _entry_B_matrices():
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	return A_train, A_test


def test_entry_point_B_adaptive_metrics(gpu, tmp_path, caplog):
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.harness import ADAPTIVE_PREFIX
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	assert ADAPTIVE_PREFIX == NEW
	A_train, A_test = _entry_B_matrices()
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	top_k, retr, ancs = [1, 10, 50], [5, 10, 50, 580], [10, 20, 30]      # 5 is odd; 580 + 30 > 600 items: over the limit at 30 anchors only
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			  "--train_data_file", str(tmp_path / "train.pkl"), "--n_seeds", "2", "--top_k_vals", "1,10,50", "--top_k_retr_vals", "5,10,50,580",
			  "--n_ent_anchors_vals", "10,20,30", "--pinv", "numpy"]
	f_old = epB.main(common + ["--misc", "old"])
	f_one = epB.main(common + ["--misc", "one", "--adaptive_rounds", "1"])
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		f_new = epB.main(common + ["--misc", "new", "--adaptive_rounds", "2"])
	txt_old, txt_one = open(f_old).read(), open(f_one).read()
	assert txt_one.replace('"misc": "one"', '"misc": "old"') == txt_old                      # N = 1 writes what no flag writes
	old, new = json.load(open(f_old)), json.load(open(f_new))
	assert "adaptive_rounds" not in old["other_args"] and new["other_args"]["adaptive_rounds"] == 2
	At_dev, Atr_dev = A_test.cuda(), A_train.cuda()
	qids = torch.arange(40, dtype=torch.int64)
	n_cells = 0
	for seed in range(2):
		rng = np.random.default_rng(seed)
		for n_anc in ancs:
			anc = sorted(rng.choice(600, size=n_anc, replace=False))
			searcher = AdaptiveSearcher(CURRowIndex(Atr_dev, np.asarray(anc), compute_dtype=None, pinv_backend="numpy"), MatrixScorer(At_dev))
			for kr in retr:
				inside = kr % 2 == 0 and kr + n_anc <= 600
				pool = searcher.search(qids, 1, kr // 2, 2, trace=True).trace[-1]["ids"].cpu().numpy() if inside else None
				for k in top_k:
					if k > kr:
						assert f"k_retvr={kr}" not in new[f"seed={seed}"].get(f"top_k={k}", {})
						continue
					o = old[f"seed={seed}"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
					n = new[f"seed={seed}"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
					assert {m: v for m, v in n.items() if not m.startswith(NEW + "~")} == o            # every old metric: equal
					new_keys = {m for m in n if m.startswith(NEW + "~")}
					if not inside:
						assert not new_keys, (k, kr, n_anc)
						continue
					assert pool.shape == (40, n_anc + kr) and all(np.isin(anc, row).all() for row in pool)
					counts = [len(set(torch.topk(A_test[q], k).indices.tolist()) & set(pool[q].tolist())) for q in range(40)]
					assert {m: n[m] for m in new_keys} == _stats(counts, k, NEW), (seed, k, kr, n_anc)
					n_cells += 1
	assert n_cells == 2 * (3 * (2 + 3 + 3) - 3)        # per seed and anchor count: k_retvr 10 (2 cells), 50 (3), 580 (3), less 580 at 30 anchors
	msgs = [r.getMessage() for r in caplog.records if NEW in r.getMessage()]
	assert len(msgs) == 2 * 3 and all("k_retvr=5: k_retvr % 2 != 0" in m for m in msgs)       # once per anchor set
	assert sum("min(600, 2048) = 600" in m for m in msgs) == 2                                # ... and the limit, at 30 anchors
