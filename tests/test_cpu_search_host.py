"""Host side of the search without the exact matrix: the argument checks of ops.rerank_scored, the cell rule and the list
layout of the pool mode, the --rerank_pool flag of both command-line entry points.  No GPU needed."""
import json

import numpy as np
import pytest
import torch

Q, N_SH, N_PQ = 4, 6, 5


def _good():
	return dict(cand=torch.arange(Q * N_PQ, dtype=torch.int32).reshape(Q, N_PQ), cand_scores=torch.zeros(Q, N_PQ),
				shared_ids=[1, 3, 4, 9, 20, 21], shared_scores=torch.zeros(Q, N_SH))


def test_rerank_scored_accepts_the_valid_forms_up_to_the_device_check():
	"""Every valid form passes the host checks and stops at the first thing that needs the GPU: CPU tensors are refused."""
	from anncur_amd import _lib, ops
	g = _good()
	for kw in (g, dict(g, shared_scores=g["shared_scores"].bfloat16()), dict(g, shared_ids=np.asarray(g["shared_ids"])), dict(g, shared_ids=torch.tensor(g["shared_ids"])),
			   dict(g, cand=ops.TopK(g["cand_scores"], g["cand"])), dict(cand=g["cand"], cand_scores=g["cand_scores"]),
			   dict(shared_ids=g["shared_ids"], shared_scores=g["shared_scores"]), dict(g, shared_ids=ops.shared_id_list(g["shared_ids"], "cpu"))):
		for k in (1, N_SH + N_PQ if "cand" in kw and "shared_ids" in kw else min(N_SH, N_PQ)):
			with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):
				ops.rerank_scored(k, **kw)
	Qa, n_sh, n_pq, cand = ops._rerank_scored_args(3, ops.TopK(g["cand_scores"], g["cand"]), g["cand_scores"], g["shared_ids"], g["shared_scores"])
	assert (Qa, n_sh, n_pq) == (Q, N_SH, N_PQ) and cand is g["cand"]
	sh = ops.shared_id_list(np.array([0, 5, 2 ** 31 - 1]), "cpu")
	assert sh.n == 3 and sh.ids.dtype == torch.int32 and sh.ids.tolist() == [0, 5, 2 ** 31 - 1] and ops.shared_id_list(sh, "cpu") is sh
	assert ops.shared_id_list([], "cpu").n == 0


@pytest.mark.parametrize("ids,msg", [([3, 1, 4], r"strictly ascending \(ids\[0\] = 3, ids\[1\] = 1\)"), ([1, 3, 3, 9], r"strictly ascending \(ids\[1\] = 3, ids\[2\] = 3\)"),
									 ([-1, 2], "negative id -1"), ([1, 2 ** 31], "beyond int32"), ([[1, 2], [3, 4]], "flat list"), ([0.5, 1.5], "integer item ids"),
									 (list(range(65536)), "above the limit of 65535")])
def test_shared_ids_are_checked_not_sorted(ids, msg):
	from anncur_amd import ops
	with pytest.raises(ValueError, match=msg):
		ops.shared_id_list(np.asarray(ids), "cpu")
	n = len(ids)
	if np.asarray(ids).ndim == 1:
		with pytest.raises(ValueError, match=msg):
			ops.rerank_scored(1, shared_ids=ids, shared_scores=torch.zeros(Q, n))


def test_rerank_scored_refuses_every_bad_shape_dtype_and_limit():
	from anncur_amd import _lib, ops
	g = _good()
	big = _lib.MAX_TOPK + 1
	bad = [
		(dict(g, cand_scores=None), "cand and cand_scores come together"),
		(dict(g, cand=None), "cand and cand_scores come together"),
		(dict(g, shared_scores=None), "shared_ids and shared_scores come together"),
		(dict(g, shared_ids=None), "shared_ids and shared_scores come together"),
		(dict(cand=None, cand_scores=None, shared_ids=None, shared_scores=None), "the pool is empty"),
		(dict(shared_ids=[], shared_scores=torch.zeros(Q, 0)), "the pool is empty"),
		(dict(g, cand_scores=torch.zeros(Q, N_PQ + 1)), "one shape"),
		(dict(g, cand=g["cand"][0], cand_scores=g["cand_scores"][0]), "2-D tensors"),
		(dict(g, cand=g["cand"].numpy()), "2-D tensors"),
		(dict(g, cand=g["cand"].long()), r"int32 ids \(got torch.int64\)"),
		(dict(g, cand_scores=g["cand_scores"].bfloat16()), r"float32 \(got torch.bfloat16\)"),
		(dict(g, shared_scores=torch.zeros(Q, N_SH + 1)), rf"\[Q x {N_SH}\]"),
		(dict(g, shared_scores=torch.zeros(Q * N_SH)), rf"\[Q x {N_SH}\]"),
		(dict(g, shared_scores=torch.zeros(Q, N_SH, dtype=torch.float64)), "float32 or bfloat16"),
		(dict(g, shared_scores=torch.zeros(Q + 1, N_SH)), rf"{Q + 1} rows, cand has {Q}"),
		(dict(cand=torch.zeros((Q, big), dtype=torch.int32), cand_scores=torch.zeros(Q, big)), rf"{big} candidates per query, above the limit of ANNCUR_MAX_TOPK = {_lib.MAX_TOPK}"),
		(dict(shared_ids=list(range(65536)), shared_scores=torch.zeros(1, 65536)), "65536 shared ids, above the limit of 65535"),
	]
	for kw, msg in bad:
		with pytest.raises(ValueError, match=msg):
			ops.rerank_scored(1, **kw)
	pool = N_SH + N_PQ
	for k in (0, -1, pool + 1, 2.0, True, None):
		with pytest.raises(ValueError, match=rf"k = {k} outside 1\.\.min\(pool size, ANNCUR_MAX_TOPK\) = min\({pool}, {_lib.MAX_TOPK}\) = {pool}"):
			ops.rerank_scored(k, **g)
	with pytest.raises(ValueError, match=rf"min\({N_PQ}, {_lib.MAX_TOPK}\) = {N_PQ}"):
		ops.rerank_scored(N_PQ + 1, g["cand"], g["cand_scores"])
	wide = dict(cand=torch.zeros((1, 2048), dtype=torch.int32), cand_scores=torch.zeros(1, 2048), shared_ids=list(range(3000)), shared_scores=torch.zeros(1, 3000))
	with pytest.raises(ValueError, match=rf"min\(5048, {_lib.MAX_TOPK}\) = {_lib.MAX_TOPK}"):
		ops.rerank_scored(_lib.MAX_TOPK + 1, **wide)
	with pytest.raises(_lib.AnncurHipError):                                  # k at the limit passes the host checks
		ops.rerank_scored(_lib.MAX_TOPK, **wide)
	with pytest.raises(_lib.AnncurHipError):
		ops.gather_pairs(torch.zeros(2, 3), torch.zeros((2, 2), dtype=torch.int32))


def test_searcher_limits_are_host_checks():
	"""CrossEncoderSearcher.search raises before the scorer is called; construction checks the anchor ids once."""
	from anncur_amd import _lib, ops
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import CrossEncoderSearcher, SearchResult
	index = CURRowIndex.__new__(CURRowIndex)                                   # (the limits need the item count and the anchor ids only)
	index.R, index.m, index.col_idxs = torch.zeros(2, 5000), 5000, [2, 5, 700, 4999]
	calls = []
	scorer = lambda q, i: calls.append(1)
	s = CrossEncoderSearcher(index, scorer)
	assert s.kc == 4 and s._shared.ids.tolist() == [2, 5, 700, 4999] and s._excl.off is None and s._excl.e_max == 4 and s._anchor_ids.dtype == torch.int32
	with pytest.raises(ValueError, match=r"2045 \+ 4 = 2049 candidates per query.*min\(5000, 2048\) = 2048.*rebuild the index without those items"):
		s.search(np.arange(3), 10, 2045)
	with pytest.raises(ValueError, match=r"min\(104, 2048\) = 104 \(got k = 105, k_retvr = 100\)"):
		s.search(np.arange(3), 105, 100)
	with pytest.raises(ValueError, match=r"min\(100, 2048\) = 100"):
		CrossEncoderSearcher(index, scorer, anchors_in_pool=False).search(np.arange(3), 101, 100)
	with pytest.raises(ValueError, match="k_retvr >= 1"):
		s.search(np.arange(3), 1, 0)
	assert calls == [] and SearchResult._fields == ("values", "indices", "n_scored")
	index.col_idxs = [5, 2, 700]
	with pytest.raises(ValueError, match="strictly ascending"):
		CrossEncoderSearcher(index, scorer)
	assert CrossEncoderSearcher(index, scorer, anchors_in_pool=False)._shared is None   # the plain mode does not need the order
	index.col_idxs = [5, 5000]
	with pytest.raises(IndexError):
		CrossEncoderSearcher(index, scorer)


def test_pool_cell_rule_pairs_and_list_layout():
	from anncur_amd import _lib, retrieval
	assert retrieval.POOL_PREFIX == "exact_vs_reranked_approx_retvr_w_anchors"
	assert retrieval.pool_cell_limit(600) == 600 and retrieval.pool_cell_limit(10 ** 6) == _lib.MAX_TOPK == 2048
	cells = [(1, 5), (10, 50), (10, 570), (50, 571), (1, 2048)]
	assert retrieval.split_pool_cells(cells, 30, 600) == ([(1, 5), (10, 50), (10, 570)], [(50, 571), (1, 2048)])       # k_retvr + n_anc <= n_ent
	assert retrieval.split_pool_cells(cells, 0, 10 ** 6) == (cells, [])
	assert retrieval.split_pool_cells(cells, 1, 10 ** 6) == (cells[:4], [(1, 2048)])                                # ... and <= ANNCUR_MAX_TOPK
	assert retrieval.split_pool_cells(cells, 2048, 10 ** 6) == ([], cells)
	assert retrieval.pool_pairs([(1, 5), (10, 50)], 30) == [(1, 35), (10, 80)]
	retrieved = torch.tensor([[7, 8, 9], [4, 5, -1]], dtype=torch.int32)
	got = retrieval.pool_list(np.array([2, 30], dtype=np.int64), retrieved)
	assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [[2, 30, 7, 8, 9], [2, 30, 4, 5, -1]]   # the anchors come first
	assert retrieval.pool_list([], retrieved.long()).tolist() == retrieved.tolist()
	# the closed form on plain arrays: the prefix n_anc + k_retvr of the list is the pool of the cell
	exact = [[9, 2, 1], [5, 3, 30]]
	for (k, kr), want in (((1, 1), [0, 0]), ((2, 1), [1, 0]), ((2, 3), [2, 1]), ((3, 2), [1, 2])):
		(ka, kb), = retrieval.pool_pairs([(k, kr)], 2)
		assert [len(set(e[:ka]) & set(row[:kb])) for e, row in zip(exact, got.tolist())] == want


def test_harness_refuses_an_unknown_pool():
	from anncur_amd import harness
	assert harness.RERANK_POOLS == ("retrieved", "retrieved+anchors")
	assert harness._check_rerank_pool("retrieved") is False and harness._check_rerank_pool("retrieved+anchors") is True
	with pytest.raises(ValueError, match="rerank_pool = anchors not supported"):
		harness._check_rerank_pool("anchors")


def test_both_parsers_take_rerank_pool():
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	for p, base in ((epA.build_parser(), ["--res_dir", "r"]), (epB.build_parser(), ["--res_dir", "r", "--test_data_file", "t"])):
		assert p.parse_args(base).rerank_pool == "retrieved"
		assert p.parse_args(base + ["--rerank_pool", "retrieved+anchors"]).rerank_pool == "retrieved+anchors"
		with pytest.raises(SystemExit):
			p.parse_args(base + ["--rerank_pool", "anchors"])


@pytest.fixture
def fake_harness(monkeypatch):
	"""The harness with its device work replaced: the score pickles are small arrays, matrices stay on the host, the evaluation calls are recorded."""
	from anncur_amd import harness
	seen = []
	scores = np.zeros((6, 40), dtype=np.float32)
	monkeypatch.setattr(harness, "load_score_pickle", lambda path: {"ment_to_ent_scores": scores, "ment_idxs": list(range(6))})
	monkeypatch.setattr(harness, "to_device_matrix", lambda s, device, dtype="fp32": s)
	monkeypatch.setattr(harness, "run_entry_A", lambda *a, **kw: seen.append(("A", a, kw)) or {})
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(("B", a, kw)) or {})
	monkeypatch.setattr(harness, "run_eval_method_fixed_anc_ent_cur", lambda *a, **kw: seen.append(("B_fixed", a, kw)) or {})
	monkeypatch.setattr(harness, "run_eval_method_embeds", lambda *a, **kw: seen.append(("B_embeds", a, kw)) or {})
	return seen, scores


def test_entry_point_A_default_builds_the_call_it_built_before(fake_harness, tmp_path):
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	seen, scores = fake_harness
	base = ["--data_name", "yugioh", "--res_dir", str(tmp_path), "--n_ment", "6", "--n_seeds", "2", "--disable_wandb", "1", "--device", "cpu", "--plot_only", "0"]
	out = epA.main(base)
	(_, args, kw), = seen
	assert kw == {} and len(args) == 6 and args[0] is scores and args[2] == 2 and args[4:] == ("auto", None)     # (A_dev, grids, n_seeds, progress, pinv, compute_dtype)
	with open(f"{out}/retrieval_wrt_exact_crossenc.json") as f:
		assert "rerank_pool" not in json.load(f)["other_args"]["arg_dict"]
	assert epA.main(base + ["--rerank_pool", "retrieved"]) == out and seen[1][2] == {}
	out = epA.main(base + ["--rerank_pool", "retrieved+anchors", "--misc", "pool"])
	assert seen[2][1][2:3] + seen[2][1][4:] == (2, "auto", None) and seen[2][2] == {"rerank_pool": "retrieved+anchors"}
	with open(f"{out}/retrieval_wrt_exact_crossenc.json") as f:
		assert json.load(f)["other_args"]["arg_dict"]["rerank_pool"] == "retrieved+anchors"


def test_entry_point_B_default_builds_the_call_it_built_before(fake_harness, tmp_path):
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	seen, scores = fake_harness
	base = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path), "--test_data_file", "test.pkl", "--train_data_file", "train.pkl", "--device", "cpu"]
	res_file = epB.main(base + ["--misc", "old"])
	(_, args, kw), = seen
	assert len(args) == 4 and args[0] is scores and args[1] is scores and args[2] == 0 and set(kw) == {"compute_dtype", "progress", "pinv_backend"}
	assert kw["compute_dtype"] is None and kw["pinv_backend"] == "auto"
	with open(res_file) as f:
		assert "rerank_pool" not in json.load(f)["other_args"]
	res_file = epB.main(base + ["--misc", "new", "--rerank_pool", "retrieved+anchors"])
	assert set(seen[1][2]) == {"compute_dtype", "progress", "pinv_backend", "rerank_pool"} and seen[1][2]["rerank_pool"] == "retrieved+anchors"
	with open(res_file) as f:
		assert json.load(f)["other_args"]["rerank_pool"] == "retrieved+anchors"
