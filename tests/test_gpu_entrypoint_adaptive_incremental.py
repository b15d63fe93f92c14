"""--adaptive_incremental through entry point B, on the small synthetic pickles of tests/test_gpu_entrypoint_adaptive.py (built
here the same way; 60 training queries = kq): with --adaptive_rounds 2 the flag writes the SAME keys as the run without it for every cell
inside its limit n_anc + k_retvr / 2 <= 60, every statistic under the adaptive prefix equals the closed form |exact[:k] & pool| recomputed
from a direct AdaptiveSearcher(incremental=True) run, the cells beyond the limit are left out and logged with the remedy, and every other
metric is untouched.  Needs an MI355X."""
import json
import logging
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW = "exact_vs_reranked_adaptive_retvr"


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


def test_entry_point_B_incremental_writes_the_same_keys(gpu, tmp_path, caplog):
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	top_k, retr, ancs = [1, 10], [10, 50, 120], [10, 20]         # k_retvr = 120: n_anc + 60 > kq = 60, beyond the incremental limit only
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			  "--train_data_file", str(tmp_path / "train.pkl"), "--top_k_vals", "1,10", "--top_k_retr_vals", "10,50,120", "--n_ent_anchors_vals", "10,20",
			  "--pinv", "numpy", "--adaptive_rounds", "2"]
	off = json.load(open(epB.main(common + ["--misc", "off"])))
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		on = json.load(open(epB.main(common + ["--misc", "on", "--adaptive_incremental"])))
	assert "adaptive_incremental" not in off["other_args"] and on["other_args"]["adaptive_incremental"] is True
	At_dev, Atr_dev = A_test.cuda(), A_train.cuda()
	qids = torch.arange(40, dtype=torch.int64)
	rng = np.random.default_rng(0)
	n_cells = 0
	for n_anc in ancs:
		anc = sorted(rng.choice(600, size=n_anc, replace=False))
		searcher = AdaptiveSearcher(CURRowIndex(Atr_dev, np.asarray(anc), compute_dtype=None, pinv_backend="numpy"), MatrixScorer(At_dev), incremental=True)
		for kr in retr:
			inside = n_anc + kr // 2 <= 60
			pool = searcher.search(qids, 1, kr // 2, 2, trace=True).trace[-1]["ids"].cpu().numpy() if inside else None
			for k in top_k:
				a = off["seed=0"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
				b = on["seed=0"][f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m=60_anc_n_e={n_anc}"]
				assert {m: v for m, v in b.items() if not m.startswith(NEW + "~")} == {m: v for m, v in a.items() if not m.startswith(NEW + "~")}
				assert any(m.startswith(NEW + "~") for m in a)                                   # the default run holds every one of these cells
				if not inside:
					assert not any(m.startswith(NEW + "~") for m in b), (k, kr, n_anc)
					continue
				assert set(b) == set(a)                                                          # the same output keys
				assert pool.shape == (40, n_anc + kr)
				counts = [len(set(torch.topk(A_test[q], k).indices.tolist()) & set(pool[q].tolist())) for q in range(40)]
				assert {m: b[m] for m in b if m.startswith(NEW + "~")} == _stats(counts, k, NEW), (k, kr, n_anc)
				n_cells += 1
	assert n_cells == 2 * 2 * 2
	msgs = [r.getMessage() for r in caplog.records if NEW in r.getMessage()]
	assert len(msgs) == 2 and all("k_retvr=120" in m and "use incremental=False" in m for m in msgs)      # once per anchor set
