"""Host side of the ranks of given items: the NumPy restatement of the contract (tests/rank_numpy.py) against a double
loop, retrieval.overlap_from_ranks / rank_curve against hand-computed cases, the documented errors of the ops before any device call, the
new symbols in the header, the binding and the built library, the static walks of `make verify` over the new code object (its kernels use no
scratch), and --rank_metrics of entry point B with its arg-dict rule.  No GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import rank_numpy as rn  # noqa: E402

NEW_SYMBOLS = ("anncur_rank_in_rows", "anncur_score_rank", "anncur_score_rank_workspace_bytes")


# ------------------------------------------------------------------ the restatement
def test_rank_ref_equals_the_double_loop_on_tie_heavy_rows():
	rng = np.random.default_rng(0)
	for Q, I, t in ((1, 1, 1), (3, 7, 7), (4, 33, 50), (2, 200, 64)):
		S = rng.integers(-3, 4, (Q, I)).astype(np.float32)
		ids = rng.integers(-1, I, (Q, t)).astype(np.int32)            # holes and duplicates
		if I > 10:
			S[0, 3:6] = np.nan
			S[Q - 1, 1], S[Q - 1, 2], S[Q - 1, 7], S[Q - 1, 8] = np.inf, -np.inf, -0.0, 0.0
			ids[0, 0], ids[Q - 1, :4] = 4, (1, 2, 7, 8)
		got = rn.rank_ref(S, ids)
		assert got.dtype == np.int32 and np.array_equal(got, rn.rank_brute(S, ids)), (Q, I, t)
		assert ((got == -1) == ((ids < 0) | np.isnan(np.take_along_axis(S, np.maximum(ids, 0).astype(np.int64), 1)))).all()


def test_rank_ref_hand_cases():
	S = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.nan, 2.0]], dtype=np.float32)
	ids = np.array([[1, 2, 6, 0, 3, 4, 5, -1, 2]], dtype=np.int32)
	#               3.0 first by id, then 3.0, 2.0, 1.0, the zeros tie (id 3 before id 4), NaN target and hole -> -1, duplicate id repeats
	assert rn.rank_ref(S, ids).tolist() == [[0, 1, 2, 3, 4, 5, -1, -1, 1]]
	# the ranks of a full permutation of a row without NaN are a permutation, and invert the stable descending argsort
	rng = np.random.default_rng(1)
	S = rng.integers(-2, 3, (5, 40)).astype(np.float32)
	order = np.argsort(-S, axis=1, kind="stable").astype(np.int32)
	assert np.array_equal(rn.rank_ref(S, order), np.tile(np.arange(40, dtype=np.int32), (5, 1)))
	assert np.array_equal(rn.bf16_round(np.array([1.0, 1.00390625, 1.01171875, -3.5], dtype=np.float32)),
						  np.array([1.0, 1.0, 1.015625, -3.5], dtype=np.float32))


# ------------------------------------------------------------------ the recall curve from ranks
def test_overlap_from_ranks_hand_cases():
	from anncur_amd.retrieval import overlap_from_ranks
	ranks = np.array([[0, 5, 2, 9], [3, -1, 0, 100], [7, 7, 7, 7]], dtype=np.int32)
	cells = [(1, 1), (2, 5), (2, 6), (4, 10), (4, 101), (3, 3), (0, 5)]
	want = [[1, 0, 0], [1, 1, 0], [2, 1, 0], [4, 2, 4], [4, 3, 4], [2, 1, 0], [0, 0, 0]]
	got = overlap_from_ranks(ranks, cells)
	assert got.dtype == np.int32 and got.shape == (7, 3) and got.tolist() == want
	assert overlap_from_ranks(torch.from_numpy(ranks), cells).tolist() == want
	with pytest.raises(ValueError, match="needs 5 ranks per query, 4 given"):
		overlap_from_ranks(ranks, [(5, 10)])
	with pytest.raises(ValueError, match="integer"):
		overlap_from_ranks(ranks.astype(np.float32), cells)


def test_rank_curve_hand_cases():
	from anncur_amd.retrieval import RANK_CURVE_RECALLS, rank_curve
	assert RANK_CURVE_RECALLS == (0.5, 0.9, 0.95, 0.99, 1.0)
	ranks = np.array([[0, 4], [1, 9], [0, 2], [3, 40], [0, 7]], dtype=np.int32)
	got = rank_curve(ranks, [1, 2])
	# top_k = 1: the five ranks 0 0 0 1 3
	assert got[1] == {"exact_topk_approx_rank~mean": 0.8, "exact_topk_approx_rank~p50": 0, "exact_topk_approx_rank~p90": 3, "exact_topk_approx_rank~p99": 3,
					  "exact_topk_approx_rank~max": 3, "k_retvr_for_recall~0.5": 1, "k_retvr_for_recall~0.9": 4, "k_retvr_for_recall~0.95": 4,
					  "k_retvr_for_recall~0.99": 4, "k_retvr_for_recall~1.0": 4}
	# top_k = 2: the ten ranks 0 0 0 1 2 3 4 7 9 40: the 5th, 9th and 10th smallest
	assert got[2] == {"exact_topk_approx_rank~mean": 6.6, "exact_topk_approx_rank~p50": 2, "exact_topk_approx_rank~p90": 9, "exact_topk_approx_rank~p99": 40,
					  "exact_topk_approx_rank~max": 40, "k_retvr_for_recall~0.5": 3, "k_retvr_for_recall~0.9": 10, "k_retvr_for_recall~0.95": 41,
					  "k_retvr_for_recall~0.99": 41, "k_retvr_for_recall~1.0": 41}
	# the product r Q k is taken exactly: 0.7 * 10 is 7, not 7.000000000000001 -> the 7th smallest, 4
	assert rank_curve(ranks, [2], recalls=(0.7, 0.1))[2]["k_retvr_for_recall~0.7"] == 5 and rank_curve(ranks, [2], recalls=(0.1,))[2]["k_retvr_for_recall~0.1"] == 1
	# a pair without a rank is never retrieved: out of mean and max, and a level that falls among such pairs is None
	got = rank_curve(np.array([[0, -1], [2, 5]], dtype=np.int32), [2], recalls=(0.5, 0.75, 1.0))[2]
	assert got["exact_topk_approx_rank~mean"] == round(7 / 3, 4) and got["exact_topk_approx_rank~max"] == 5 and got["exact_topk_approx_rank~p99"] is None
	assert (got["k_retvr_for_recall~0.5"], got["k_retvr_for_recall~0.75"], got["k_retvr_for_recall~1.0"]) == (3, 6, None)
	# the curve and the counts agree: k_retvr_for_recall~r is the smallest k_retvr whose overlap reaches ceil(r Q k)
	from anncur_amd.retrieval import overlap_from_ranks
	kr = rank_curve(ranks, [2])[2]["k_retvr_for_recall~0.9"]
	assert overlap_from_ranks(ranks, [(2, kr)]).sum() >= 9 > overlap_from_ranks(ranks, [(2, kr - 1)]).sum()
	with pytest.raises(ValueError, match="top_k = 3 needs 3 ranks per query, 2 given"):
		rank_curve(ranks, [3])


# ------------------------------------------------------------------ the documented errors, before any device call
def test_rank_ops_refuse_bad_arguments_on_the_host():
	from anncur_amd import _lib, ops
	assert ops.RANK_MAX_T == _lib.RANK_MAX_T == 1024
	S = torch.zeros(3, 50)                                     # CPU tensors: the device check would raise AnncurHipError, and comes last
	ok = torch.zeros((3, 4), dtype=torch.int32)
	Xp, Etp = torch.zeros((3, 64), dtype=torch.bfloat16), torch.zeros((64, 64), dtype=torch.bfloat16)
	calls = {"rank_in_rows": lambda ids, S=S: ops.rank_in_rows(S, ids), "score_rank": lambda ids: ops.score_rank(Xp, Etp, 50, ids),
			 "rank_dense": lambda ids: ops.rank_dense(torch.zeros(3, 8), torch.zeros(50, 8), ids)}
	for name, call in calls.items():
		with pytest.raises(ValueError, match=r"t = 0 targets per row, need 1 <= t <= 1024"):
			call(torch.zeros((3, 0), dtype=torch.int32))
		with pytest.raises(ValueError, match=r"t = 1025 targets per row, need 1 <= t <= 1024"):
			call(torch.zeros((3, 1025), dtype=torch.int32))
		for bad, word in ((50, "id 50"), (51, "id 51"), (-2, "id -2")):
			ids = ok.clone()
			ids[1, 2] = bad
			with pytest.raises(ValueError, match=word + r" is outside \[0, 50\) and is not the hole -1"):
				call(ids)
			with pytest.raises(ValueError, match=word):
				call(ids.numpy())                              # NumPy ids are checked the same way
		for wrong in (ok.long(), ok.float(), [[0, 1, 2, 3]] * 3):
			with pytest.raises(TypeError, match="ids must be int32"):
				call(wrong)
		with pytest.raises(ValueError, match=r"ids must be \[Q x t\] with Q = 3 rows"):
			call(torch.zeros((2, 4), dtype=torch.int32))
		with pytest.raises(_lib.AnncurHipError, match="no CPU fallback"):
			call(torch.tensor([[0, -1, 49, 49]] * 3, dtype=torch.int32))      # valid ids (a hole, duplicates): only the device is missing
	with pytest.raises(TypeError, match="unsupported dtype"):
		ops.rank_in_rows(S.double(), ok)
	with pytest.raises(TypeError, match="unsupported dtype"):
		ops.rank_dense(torch.zeros(3, 8).double(), torch.zeros(50, 8), ok)
	with pytest.raises(ValueError, match="2-D"):
		ops.rank_in_rows(torch.zeros(50), ok)
	with pytest.raises(TypeError, match="Xp must be packed bfloat16"):
		ops.score_rank(Xp.float(), Etp, 50, ok)
	with pytest.raises(TypeError, match="Etp must be packed bfloat16"):
		ops.score_rank(Xp, Etp.float(), 50, ok)
	for xp, etp, I in ((torch.zeros((3, 96), dtype=torch.bfloat16), torch.zeros((64, 96), dtype=torch.bfloat16), 50),     # Kp outside the four widths
					   (Xp, torch.zeros((64, 128), dtype=torch.bfloat16), 50), (Xp, torch.zeros((32, 64), dtype=torch.bfloat16), 50), (Xp, Etp, 0)):
		with pytest.raises(ValueError, match=r"Xp \[Q x Kp\], Etp \[ceil32\(I\) x Kp\]"):
			ops.score_rank(xp, etp, I, ok)
	assert [ops.score_rank_ok(kp, 100, 5) for kp in (64, 128, 256, 512, 32, 96, 640, 1024)] == [True] * 4 + [False] * 4
	assert [ops.score_rank_ok(64, 100, t) for t in (0, 1, 1024, 1025)] == [False, True, True, False]
	assert not ops.score_rank_ok(64, 0, 1) and not ops.score_rank_ok(64, 2 ** 31, 1)


def test_index_classes_take_int64_ids_and_refuse_the_rest():
	from anncur_amd.cur import _rank_ids_arg
	dev = torch.device("cpu")
	got = _rank_ids_arg(np.array([[0, 5, -1]], dtype=np.int64), dev)
	assert got.dtype == torch.int32 and got.tolist() == [[0, 5, -1]] and got.is_contiguous()
	assert _rank_ids_arg(torch.arange(12, dtype=torch.int32).reshape(3, 4)[:, :2], dev).is_contiguous()
	with pytest.raises(ValueError, match="is no item id"):
		_rank_ids_arg(np.array([[2 ** 31]], dtype=np.int64), dev)
	with pytest.raises(ValueError, match="is no item id"):
		_rank_ids_arg(np.array([[-2]], dtype=np.int64), dev)
	with pytest.raises(TypeError, match="int32 or int64"):
		_rank_ids_arg(np.zeros((1, 2), dtype=np.float32), dev)
	with pytest.raises(ValueError, match=r"\[Q x t\]"):
		_rank_ids_arg(np.zeros(4, dtype=np.int32), dev)


# ------------------------------------------------------------------ header, binding, library
def test_new_symbols_in_header_binding_and_library():
	from anncur_amd import _lib
	header = open(os.path.join(ROOT, "include", "anncur_hip.h")).read()
	lib = _lib.load()
	exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
	for name, n_args in zip(NEW_SYMBOLS, (10, 14, 4)):
		assert re.search(r"\b" + name + r"\(", header), name
		assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
		assert re.search(r" T " + name + r"$", exported, re.M), name
	assert re.search(r"#define ANNCUR_RANK_MAX_T 1024\b", header)
	for phrase in ("rank = #{ i != id : s[i] > a  or  (s[i] == a and i < id) }", "-0.0 and +0.0 tie", "NaN score is never ahead", "hole (id == -1)",
				   "Duplicate ids", "bit-identical", "are not counted", "neither store nor count", "nothing in it pre-filled"):
		assert phrase in header, phrase


def test_workspace_query_and_library_refusals_without_a_device():
	from anncur_amd import _lib
	lib = _lib.load()
	ws = lib.anncur_score_rank_workspace_bytes
	for Q, I, kp, t in ((0, 10, 64, 1), (-1, 10, 64, 1), (2 ** 31, 10, 64, 1), (5, 0, 64, 1), (5, 2 ** 31 - 65, 64, 1), (5, 10, 96, 1), (5, 10, 1024, 1), (5, 10, 64, 0),
						(5, 10, 64, 1025)):
		assert ws(Q, I, kp, t) == 0, (Q, I, kp, t)
	for Q, I, kp, t in ((1, 1, 64, 1), (70, 4101, 512, 1024), (10000, 100000, 256, 100), (2 ** 31 - 1, 2 ** 31 - 66, 128, 1024)):
		got = ws(Q, I, kp, t)
		assert got % 256 == 0 and 16 * Q * t <= got < 16 * Q * t + 256, (Q, I, kp, t, got)
	p = ctypes.c_void_p(256)

	def rows(dtype=0, Q=3, I=10, ld=10, t=2, S=p, ids=p, rank=p):
		return lib.anncur_rank_in_rows(S, dtype, Q, I, ld, ids, t, rank, None, None)
	for kw, msg in ((dict(dtype=2), b"bad dtype"), (dict(ld=9), b"bad shape"), (dict(I=0, ld=0), b"bad shape"), (dict(Q=-1), b"bad shape"), (dict(Q=2 ** 31), b"bad shape"),
					(dict(I=2 ** 31 - 1, ld=2 ** 31), b"bad shape"), (dict(t=0), b"t = 0 outside 1..1024"), (dict(t=1025), b"t = 1025 outside 1..1024"),
					(dict(S=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(rank=None), b"null pointer")):
		assert rows(**kw) == -1 and msg in lib.anncur_last_error(), (kw, lib.anncur_last_error())
	assert rows(Q=0, S=None, ids=None, rank=None) == 0                 # no rows: nothing to do, nothing read

	def fused(ldx=64, lde=64, Q=3, I=10, kp=64, t=2, X=p, Et=p, ids=p, rank=p, w=p, wb=1 << 40):
		return lib.anncur_score_rank(X, ldx, Et, lde, Q, I, kp, ids, t, rank, None, w, wb, None)
	assert fused(kp=96, ldx=96, lde=96) == -4 and b"Kp must be 64, 128, 256 or 512" in lib.anncur_last_error()
	for kw, msg in ((dict(Q=-1), b"bad shape"), (dict(I=0), b"bad shape"), (dict(I=2 ** 31 - 65), b"bad shape"), (dict(t=0), b"t = 0 outside"), (dict(t=1025), b"t = 1025 outside"),
					(dict(X=None), b"null pointer"), (dict(Et=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(rank=None), b"null pointer"),
					(dict(lde=128), b"packed bf16"), (dict(ldx=60), b"packed bf16"), (dict(ldx=68), b"packed bf16"), (dict(X=ctypes.c_void_p(264)), b"packed bf16"),
					(dict(Et=ctypes.c_void_p(264)), b"packed bf16")):
		assert fused(**kw) == -1 and msg in lib.anncur_last_error(), (kw, lib.anncur_last_error())
	for kw in (dict(w=None), dict(w=ctypes.c_void_p(264)), dict(wb=ws(3, 10, 64, 2) - 1)):
		assert fused(**kw) == -2 and b"workspace missing, misaligned or too small" in lib.anncur_last_error(), kw
	assert fused(Q=0, X=None, Et=None, ids=None, rank=None, w=None, wb=0) == 0


def test_static_walks_and_resources_of_the_new_code_object():
	"""What `make verify` runs, over the new kernels: the MFMA hazard walk finds nothing in the eight tile kernels (one MFMA per 16 of Kp,
	collect and count), and none of the new kernels uses scratch; the LDS of the one-workgroup-per-row kernels is the three arrays of
	ANNCUR_RANK_MAX_T entries the header's limit stands for.  The whole library's verdicts (all three scripts) stay clean."""
	from anncur_amd import _lib
	import check_kernel_resources as ckr
	import check_mfma_hazards as cmh
	from isa_tools import kernel_notes
	f, n_kernels, n_mfma = cmh.check(_lib.LIB_PATH, only=r"\d+rank_(collect|count)_kernel")
	assert f == [] and n_kernels == 8 and n_mfma == 2 * (4 + 8 + 16 + 32), (f, n_kernels, n_mfma)
	mine = [k for text in kernel_notes(_lib.LIB_PATH) for k in ckr.parse_kernel_notes(text) if re.search(r"\d+rank_(rows|collect|sort|count|finish)_kernel", k[".name"])]
	assert len(mine) == 2 + 4 + 1 + 4 + 1, [k[".name"] for k in mine]
	for k in mine:
		print("%-70s vgpr %3d agpr %3d lds %5d scratch %d" % (k[".name"], k[".vgpr_count"], k.get(".agpr_count", 0), k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]))
		assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k[".uses_dynamic_stack"] is False, k
		assert k[".max_flat_workgroup_size"] == 256
	lds = {re.search(r"rank_(\w+?)_kernel", k[".name"]).group(1): k[".group_segment_fixed_size"] for k in mine}
	assert lds == {"rows": 1024 * 20, "collect": 0, "sort": 1024 * 8, "count": 0, "finish": 1024 * 12}
	f, rows, _ = ckr.check(_lib.LIB_PATH)
	assert f == [] and len(rows) == 3


def test_make_verify_passes_on_the_built_library():
	from anncur_amd import _lib
	assert os.path.isfile(_lib.LIB_PATH)
	for script in ("check_mfma_hazards.py", "check_lds_hazards.py", "check_kernel_resources.py"):       # the three steps of the Makefile's verify target
		r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), _lib.LIB_PATH], capture_output=True, text=True)
		assert r.returncode == 0 and " 0 findings" in r.stdout, (script, r.stdout[-2000:], r.stderr[-2000:])
	mk = open(os.path.join(ROOT, "anncur_amd", "csrc", "Makefile")).read()
	assert re.search(r"^SRCS\s*:=.*\brank\.hip\b", mk, re.M)
	assert all(f"scripts/{s}" in mk for s in ("check_mfma_hazards.py", "check_lds_hazards.py", "check_kernel_resources.py"))


# ------------------------------------------------------------------ entry point B
def test_harness_refuses_rank_metrics_beside_adaptive_rounds():
	from anncur_amd import harness
	with pytest.raises(ValueError, match=r"rank_metrics needs adaptive_rounds = 1 \(got 2\)"):
		harness.run_eval_method_cur(torch.zeros(2, 5), torch.zeros(2, 5), 0, {"top_k_vals": [1], "top_k_retr_vals": [2], "n_ent_anchors_vals": [1]}, rank_metrics=True,
									adaptive_rounds=2)


def test_entry_point_B_flag_and_its_arg_dict_rule(tmp_path, monkeypatch):
	"""--rank_metrics: off by default and then absent from the written other_args (the default run writes what it wrote before the flag
	existed); on, it is recorded and reaches harness.run_eval_method_cur for method cur only; beside --adaptive_rounds N >= 2 it is an
	argparse error."""
	from anncur_amd import harness
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path), "--test_data_file", "t.pkl", "--train_data_file", "r.pkl"]
	parser = epB.build_parser()
	assert parser.parse_args(common).rank_metrics is False and parser.parse_args(common + ["--rank_metrics"]).rank_metrics is True
	assert parser.parse_args(common + ["--rank_metrics", "--adaptive_rounds", "1"]).rank_metrics is True
	for bad in (["--rank_metrics", "--adaptive_rounds", "2"], ["--adaptive_rounds", "4", "--rank_metrics"]):
		with pytest.raises(SystemExit):
			parser.parse_args(common + bad)
	monkeypatch.setattr(epB, "run_eval_method", lambda *a, **kw: ({}, {}))
	cpu = torch.device("cpu")
	off = json.load(open(epB.run(parser.parse_args(common + ["--misc", "off"]), cpu)))
	on = json.load(open(epB.run(parser.parse_args(common + ["--misc", "on", "--rank_metrics"]), cpu)))
	assert "rank_metrics" not in off["other_args"] and on["other_args"]["rank_metrics"] is True
	assert {k: v for k, v in on["other_args"].items() if k not in ("rank_metrics", "misc")} == {k: v for k, v in off["other_args"].items() if k != "misc"}
	monkeypatch.undo()
	seen = []
	monkeypatch.setattr(harness, "load_score_pickle", lambda f: {"ment_to_ent_scores": torch.zeros(3, 20), "ment_idxs": [0, 1, 2]})
	monkeypatch.setattr(harness, "to_device_matrix", lambda A, device, dtype: A)
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(kw) or {})
	for extra, want in (([], {}), (["--rank_metrics"], {"rank_metrics": True}), (["--rank_metrics", "--anchor_selection", "pivoted"], {"rank_metrics": True})):
		epB.run_eval_method("cur", "t.pkl", "r.pkl", parser.parse_args(common + extra), 0, cpu)
		kw = seen.pop()
		assert {k: v for k, v in kw.items() if k == "rank_metrics"} == want, (extra, kw)
