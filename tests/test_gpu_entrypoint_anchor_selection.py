"""--anchor_selection through entry point B, on the small synthetic pickles of tests/test_gpu_entrypoint_adaptive.py (built here
the same way): with pivoted the JSON keeps the default run's key layout and records the choice, the anchor sets of successive counts are
nested prefixes of ONE selection (seen by a spy on harness.CURApprox), a count above the number of training queries is left out and logged
once; with the default the file equals, byte for byte, the one written with the flag omitted.  The last test prints recall and cond(W),
random against pivoted, and asserts nothing about them.  Needs an MI355X."""
import json
import logging
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


def _entry_B_matrices():
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	return A_train, A_test


def _layout(d):
	return {k: _layout(v) for k, v in d.items()} if isinstance(d, dict) else None


def test_entry_point_B_pivoted_and_default(gpu, tmp_path, caplog, monkeypatch):
	from anncur_amd import harness, ops
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	A_train, A_test = _entry_B_matrices()
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	base = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			"--train_data_file", str(tmp_path / "train.pkl"), "--top_k_vals", "1,10", "--top_k_retr_vals", "10,50", "--pinv", "numpy"]
	f_old = epB.main(base + ["--n_ent_anchors_vals", "0,10,20,30", "--misc", "old"])
	f_rnd = epB.main(base + ["--n_ent_anchors_vals", "0,10,20,30", "--misc", "rnd", "--anchor_selection", "random"])
	assert open(f_rnd).read().replace('"misc": "rnd"', '"misc": "old"') == open(f_old).read()      # the default: byte for byte what no flag writes
	seen = []

	class Spy(harness.CURApprox):
		def __init__(self, *a, **kw):
			seen.append(list(kw["col_idxs"]))
			super().__init__(*a, **kw)
	monkeypatch.setattr(harness, "CURApprox", Spy)
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		f_new = epB.main(base + ["--n_ent_anchors_vals", "0,10,20,30,70", "--misc", "new", "--anchor_selection", "pivoted"])   # 70 > kq = 60 training queries
	old, new = json.load(open(f_old)), json.load(open(f_new))
	assert "anchor_selection" not in old["other_args"] and new["other_args"]["anchor_selection"] == "pivoted"
	assert {k: v for k, v in new["other_args"].items() if k not in ("anchor_selection", "misc", "n_ent_anchors_vals", "retriever_params")} == \
		{k: v for k, v in old["other_args"].items() if k not in ("misc", "n_ent_anchors_vals", "retriever_params")}
	assert _layout(new["seed=0"]) == _layout(old["seed=0"]) and set(new) == set(old)               # the same cells (70 left out), the same metric names
	assert "anc_n_m=60_anc_n_e=0" in new["seed=0"]["top_k=1"]["k_retvr=10"]                        # n_anc = 0 keeps its branch
	# one selection, nested: every anchor set is the sorted prefix of the direct call's order
	ids, _, n_sel = ops.select_pivoted(A_train.cuda(), 30)
	order = ids.cpu().numpy()
	assert n_sel == 30 and [len(s) for s in seen] == [10, 20, 30]
	for s in seen:
		assert s == sorted(int(i) for i in order[:len(s)])
	assert set(seen[0]) < set(seen[1]) < set(seen[2])
	msgs = [r.getMessage() for r in caplog.records if "anchor_selection=pivoted" in r.getMessage()]
	assert len(msgs) == 1 and "n_ent_anchors 70" in msgs[0] and "min(60, 600, 2048) = 60" in msgs[0]
	# and the selection changes the numbers: the pivoted cells are not the random ones
	cell = lambda r, n: r["seed=0"]["top_k=10"]["k_retvr=50"][f"anc_n_m=60_anc_n_e={n}"]
	assert cell(new, 0) == cell(old, 0) and any(cell(new, n) != cell(old, n) for n in (10, 20, 30))


def test_run_eval_method_cur_leaves_out_counts_beyond_the_rank(gpu, caplog):
	"""Exact integer rank 8: the selection stops at n_sel = 8, the counts 10 and 20 are left out and logged once, 4 and 8 run."""
	from anncur_amd import harness
	rng = np.random.default_rng(8)
	A = (rng.integers(-3, 4, (50, 8)) @ rng.integers(-3, 4, (8, 400))).astype(np.float32)
	assert np.linalg.matrix_rank(A.astype(np.float64)) == 8
	A_train, A_test = torch.from_numpy(A[:30]).cuda(), torch.from_numpy(A[30:]).cuda()
	grids = {"top_k_vals": [1, 5], "top_k_retr_vals": [20], "n_ent_anchors_vals": [4, 8, 10, 20]}
	with caplog.at_level(logging.INFO, logger="anncur_amd.harness"):
		res = harness.run_eval_method_cur(A_test, A_train, 0, grids, pinv_backend="numpy", anchor_selection="pivoted")
	assert sorted(res["top_k=5"]["k_retvr=20"]) == ["anc_n_m=30_anc_n_e=4", "anc_n_m=30_anc_n_e=8"]
	msgs = [r.getMessage() for r in caplog.records if "anchor_selection=pivoted" in r.getMessage()]
	assert len(msgs) == 1 and "n_ent_anchors 10,20" in msgs[0] and "n_sel = 8" in msgs[0]


def test_recall_and_cond_random_against_pivoted_are_printed(gpu):
	"""A record, not a gate: DESIGN 4.4d's small setting -- rank 12 + 0.4 noise, kq = 256, m = 6000, 24 anchors, 48 test queries --
	through CURRowIndex.topk (k_retvr = 48, recall@10 of the retrieved list) and through AdaptiveSearcher at the budget 24 + 48 in 1 / 2 / 4 rounds."""
	from anncur_amd.cur import CURRowIndex, select_anchor_items
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	Q, m, kq, kc, rank = 48, 6000, 256, 24, 12
	rng = np.random.default_rng(1)
	A = (rng.standard_normal((kq + Q, rank)) @ rng.standard_normal((rank, m)) / np.sqrt(rank) + 0.4 * rng.standard_normal((kq + Q, m))).astype(np.float32)
	R, At = torch.from_numpy(A[:kq]).cuda(), torch.from_numpy(A[kq:]).cuda()
	exact = np.argsort(-A[kq:], axis=1, kind="stable")[:, :10]
	recall = lambda got: np.mean([np.isin(exact[q], got[q]).mean() for q in range(Q)])
	sets = {"random": select_anchor_items(R, kc, method="random", rng=np.random.default_rng(2)).sorted(kc), "pivoted": select_anchor_items(R, kc).sorted(kc)}
	for name, anc in sets.items():
		assert len(anc) == kc
		index = CURRowIndex(R, np.asarray(anc), compute_dtype="fp32", pinv_backend="numpy")
		line = [f"cond(W) = {np.linalg.cond(A[:kq][:, anc].astype(np.float64)):.1f}",
				f"topk recall@10 of 48 retrieved = {recall(index.topk(At[:, anc].contiguous(), 48).indices.cpu().numpy()):.4f}"]
		for n_rounds in (1, 2, 4):
			res = AdaptiveSearcher(index, MatrixScorer(At)).search(torch.arange(Q, dtype=torch.int64), 10, 48 // n_rounds, n_rounds)
			line.append(f"adaptive {n_rounds} round(s) = {recall(res.indices.cpu().numpy()):.4f}")
		print(f"{name} anchors: " + ", ".join(line))
