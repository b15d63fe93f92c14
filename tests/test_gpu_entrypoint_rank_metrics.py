"""--rank_metrics through entry point B, on a small synthetic pickle (60 test queries, 1500 items, fp32, --pinv numpy):
without the flag the file has no approx_rank key and no trace of the flag; with it every pre-existing key and value is unchanged, the
counts retrieval.overlap_from_ranks derives from the ranks reproduce every reported (top_k, k_retvr) cell exactly, and
k_retvr_for_recall~1.0 - 1 is the largest rank.  Needs an MI355X."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _has_key(d, key):
	return isinstance(d, dict) and (key in d or any(_has_key(v, key) for v in d.values()))


def test_entry_point_B_rank_metrics(gpu, tmp_path, monkeypatch):
	from anncur_amd import harness
	from anncur_amd.eval_utils import flatten_overlap, overlap_stats_from_counts
	from anncur_amd.retrieval import overlap_from_ranks
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(5)
	Z = torch.randn(16, 1500, generator=g)
	A_train = torch.randn(80, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(80, 1500, generator=g)
	A_test = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 1500, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(80)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(80, 140)))
	base = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			"--train_data_file", str(tmp_path / "train.pkl"), "--top_k_vals", "1,10,50", "--top_k_retr_vals", "10,50,100,500", "--n_ent_anchors_vals", "0,20,50",
			"--pinv", "numpy"]
	off = json.load(open(epB.main(base + ["--misc", "off"])))
	seen = {}
	put = harness._put_rank_metrics
	monkeypatch.setattr(harness, "_put_rank_metrics", lambda res, ranks, top_k_vals, k_max, anc_key: (seen.__setitem__(anc_key, ranks.cpu().numpy()),
																									  put(res, ranks, top_k_vals, k_max, anc_key))[1])
	on = json.load(open(epB.main(base + ["--misc", "on", "--rank_metrics"])))
	# without the flag: today's layout, no trace of the feature
	assert not _has_key(off, "approx_rank") and "rank_metrics" not in off["other_args"]
	assert sorted(off["seed=0"]) == ["top_k=1", "top_k=10", "top_k=50"] and sorted(off["seed=0"]["top_k=10"]) == ["k_retvr=10", "k_retvr=100", "k_retvr=50", "k_retvr=500"]
	# with it: everything that was there is unchanged
	assert on["other_args"]["rank_metrics"] is True
	stripped = copy.deepcopy(on)
	del stripped["other_args"]["rank_metrics"]
	stripped["other_args"]["misc"] = "off"
	for k in (1, 10, 50):
		del stripped["seed=0"][f"top_k={k}"]["approx_rank"]
	assert stripped == off
	anc_keys = ["anc_n_m=80_anc_n_e=0", "anc_n_m=80_anc_n_e=20", "anc_n_m=80_anc_n_e=50"]
	assert sorted(seen) == anc_keys
	for k in (1, 10, 50):
		got = on["seed=0"][f"top_k={k}"]["approx_rank"]
		assert sorted(got) == anc_keys
		for anc in anc_keys:
			ranks = seen[anc]
			assert ranks.shape == (60, 50) and ranks.dtype == np.int32 and (ranks >= 0).all() and (ranks < 1500).all()
			m = got[anc]
			assert sorted(m) == sorted([f"exact_topk_approx_rank~{s}" for s in ("mean", "p50", "p90", "p99", "max")] +
									   [f"k_retvr_for_recall~{r}" for r in (0.5, 0.9, 0.95, 0.99, 1.0)])
			assert m["k_retvr_for_recall~1.0"] - 1 == m["exact_topk_approx_rank~max"] == int(ranks[:, :k].max())
			assert m["exact_topk_approx_rank~mean"] == round(float(ranks[:, :k].mean()), 4)
			# the ranks reproduce every reported cell: the counts, hence every statistic the file holds
			cells = [(k, kr) for kr in (10, 50, 100, 500) if k <= kr]
			counts = overlap_from_ranks(ranks, cells)
			for j, (_, kr) in enumerate(cells):
				assert flatten_overlap(overlap_stats_from_counts(counts[j], k)) == on["seed=0"][f"top_k={k}"][f"k_retvr={kr}"][anc], (k, kr, anc)
			# and the recall levels are the curve's: the smallest k_retvr whose lists hold that share of the exact top-k items
			for r in (0.5, 0.9, 0.99):
				kr = m[f"k_retvr_for_recall~{r}"]
				need = -(-int(r * 100) * 60 * k // 100)
				assert overlap_from_ranks(ranks, [(k, kr)]).sum() >= need > overlap_from_ranks(ranks, [(k, kr - 1)]).sum(), (k, anc, r)
	# no anchors: every score ties, an item's rank is its id
	from anncur_amd import ops
	exact = ops.rowwise_topk(A_test.cuda(), 50).indices.cpu().numpy()
	assert np.array_equal(seen[anc_keys[0]], exact)
