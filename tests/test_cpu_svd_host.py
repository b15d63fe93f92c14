"""The host side of the Jacobi SVD route without a GPU: every limit and every flag rule is an error that names what it guards,
raised before anything is launched; both CLIs take --pinv svd / --pinv_rcond and keep the written other_args of a default run as it was."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_functions_and_limits_are_bound():
	from anncur_amd import _lib
	names = ("anncur_svd_workspace_bytes", "anncur_svd_init", "anncur_svd_sweep", "anncur_svd_finish", "anncur_svd_scale_cols")
	src = open(os.path.join(ROOT, "include", "anncur_hip.h")).read()
	lib = _lib.load()
	for name in names:
		assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, src)
	assert int(re.search(r"#define ANNCUR_SVD_MAX_G\s+(\d+)", src).group(1)) == _lib.SVD_MAX_G == 2048
	assert int(re.search(r"#define ANNCUR_SVD_MAX_L\s+(\d+)", src).group(1)) == _lib.SVD_MAX_L == 8192
	# the workspace: H [g x Lp] + Vt [g x gp] doubles, pitches rounded up to 32; 0 outside the limits (pure host arithmetic)
	assert lib.anncur_svd_workspace_bytes(96, 96) == 8 * (96 * 96 + 96 * 96)
	assert lib.anncur_svd_workspace_bytes(257, 130) == lib.anncur_svd_workspace_bytes(130, 257) == 8 * (130 * 288 + 130 * 160)
	assert lib.anncur_svd_workspace_bytes(1, 1) == 8 * (32 + 32)
	assert lib.anncur_svd_workspace_bytes(2048, 8192) == 8 * (2048 * 8192 + 2048 * 2048)
	for bad in ((0, 5), (5, 0), (2049, 2049), (8193, 4), (4, 8193)):
		assert lib.anncur_svd_workspace_bytes(*bad) == 0
	# the C entry points refuse the same shapes with ANNCUR_E_INVALID and a message, before any pointer is read
	assert lib.anncur_svd_sweep(2049, 2049, None, 0, None, None) == -1
	assert b"ANNCUR_SVD_MAX_G = 2048" in lib.anncur_last_error()
	assert lib.anncur_svd_init(None, 0, 4, 8193, 4, None, 0, None) == -1
	assert b"ANNCUR_SVD_MAX_L = 8192" in lib.anncur_last_error()
	assert lib.anncur_svd_finish(8, 4, None, 0, None, None, 4, None, 4, None, None) == -2      # a missing workspace: ANNCUR_E_WORKSPACE


def test_svd_jacobi_limits_are_value_errors_before_any_launch():
	from anncur_amd import ops, pinv
	with pytest.raises(ValueError, match=r"min\(rows, cols\) = 2049 outside 1\.\.ANNCUR_SVD_MAX_G = 2048"):
		ops.svd_jacobi(torch.empty(2049, 2049))
	with pytest.raises(ValueError, match=r"max\(rows, cols\) = 8193 above ANNCUR_SVD_MAX_L = 8192"):
		ops.svd_jacobi(torch.empty(8193, 3))
	with pytest.raises(ValueError, match=r"max\(rows, cols\) = 8193 above ANNCUR_SVD_MAX_L = 8192"):
		ops.svd_jacobi(torch.empty(3, 8193))
	with pytest.raises(ValueError, match=r"min\(rows, cols\) = 0 outside 1\.\.ANNCUR_SVD_MAX_G"):
		ops.svd_jacobi(torch.empty(0, 7))
	with pytest.raises(ValueError, match="2-D tensor"):
		ops.svd_jacobi(torch.empty(7))
	for bad in (0, -1, 2.5, True):
		with pytest.raises(ValueError, match="max_sweeps must be an integer >= 1"):
			ops.svd_jacobi(torch.empty(4, 4), max_sweeps=bad)
	# inside the limits the next thing in the way is the missing GPU: no CPU path
	with pytest.raises(Exception, match="need tensors on the GPU"):
		ops.svd_jacobi(torch.zeros(4, 4))
	# rcond: [0, 1), checked before the decomposition is looked at
	for bad, shown in ((1, "1"), (1.0, "1.0"), (-0.1, "-0.1"), (float("nan"), "nan"), (2, "2")):
		with pytest.raises(ValueError, match=r"pinv_from_svd: rcond = %s outside \[0, 1\)" % re.escape(shown)):
			ops.pinv_from_svd(None, rcond=bad)
		with pytest.raises(ValueError, match=r"pinv_svd: rcond = %s outside \[0, 1\)" % re.escape(shown)):
			pinv.pinv_svd(torch.zeros(4, 4), rcond=bad)
	with pytest.raises(ValueError, match="rcond must be a number"):
		ops.pinv_from_svd(None, rcond="tiny")


def test_pinv_backend_and_rcond_rules():
	from anncur_amd import cur
	assert cur.PINV_BACKENDS == ("auto", "device", "numpy", "device32", "svd") and cur.PINV_RCOND_BACKENDS == ("numpy", "svd")
	M, cpu = torch.eye(4), torch.device("cpu")
	for backend in ("auto", "device", "device32"):
		with pytest.raises(ValueError, match=r"rcond = 0\.01 given with pinv_backend = '%s': Newton-Schulz cannot truncate" % backend):
			cur._pinv(M, cpu, backend, 0.01)
		with pytest.raises(ValueError, match="Newton-Schulz cannot truncate"):
			cur.CURRowIndex(torch.zeros(4, 9), [0, 1, 2, 3], pinv_backend=backend, rcond=0.01)
		assert cur.check_pinv_args(backend, None) is None
	for backend in ("numpy", "svd"):
		for bad in (1, -0.1):
			with pytest.raises(ValueError, match=r"rcond = %s outside \[0, 1\)" % re.escape(repr(bad))):
				cur._pinv(M, cpu, backend, bad)
			with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
				cur.CURRowIndex(torch.zeros(4, 9), [0, 1, 2, 3], pinv_backend=backend, rcond=bad)
		assert cur.check_pinv_args(backend, 0) == 0.0 and cur.check_pinv_args(backend, 0.25) == 0.25
	with pytest.raises(ValueError, match="pinv_backend = qr not supported"):
		cur._pinv(M, cpu, "qr")
	# a block outside the decomposition's limits names them (the oracle's tall C and long R end here)
	with pytest.raises(ValueError, match=r"ANNCUR_SVD_MAX_L = 8192 \(block 9000 x 5\)"):
		cur._pinv(torch.zeros(9000, 5), cpu, "svd")
	with pytest.raises(ValueError, match=r"ANNCUR_SVD_MAX_G = 2048"):
		cur._pinv(torch.zeros(2049, 2100), cpu, "svd", 0.01)
	# "numpy" leaves the default call as it was (the reference's fp32 call, bit for bit) and passes a given rcond on to numpy.linalg.pinv, in
	# fp64 on the same fp32 values, rounded once: the parity reference of "svd"
	W = torch.tensor(np.random.default_rng(0).standard_normal((6, 4)).astype(np.float32) * np.array([1.0, 0.5, 1e-3, 1e-5], dtype=np.float32))
	assert torch.equal(cur._pinv(W, cpu, "numpy"), torch.from_numpy(np.linalg.pinv(W.numpy())))
	assert torch.equal(cur._pinv(W, cpu, "numpy", 1e-2), torch.from_numpy(np.linalg.pinv(W.numpy().astype(np.float64), rcond=1e-2).astype(np.float32)))
	assert cur._pinv(W, cpu, "numpy", 1e-2).dtype == torch.float32
	assert not torch.equal(cur._pinv(W, cpu, "numpy", 1e-2), cur._pinv(W, cpu, "numpy"))
	info = {"rank": 3}
	assert tuple(cur._pinv(torch.zeros(0, 5), cpu, "svd", None, info).shape) == (5, 0) and info == {"singular_values": None, "rank": None}


COMMON_B = ["--data_name", "lego", "--eval_method", "cur", "--test_data_file", "t.pkl", "--train_data_file", "r.pkl"]
COMMON_A = ["--data_name", "lego"]


@pytest.mark.parametrize("entry", ["A", "B"])
def test_both_parsers_take_svd_and_rcond(entry, tmp_path):
	if entry == "A":
		from eval import run_retrieval_eval_wrt_exact_crossenc as ep
		common = COMMON_A + ["--res_dir", str(tmp_path)]
	else:
		from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as ep
		common = COMMON_B + ["--res_dir", str(tmp_path)]
	parser = ep.build_parser()
	ns = parser.parse_args(common)
	assert ns.pinv == "auto" and ns.pinv_rcond is None
	ns = parser.parse_args(common + ["--pinv", "svd"])
	assert ns.pinv == "svd" and ns.pinv_rcond is None
	ns = parser.parse_args(common + ["--pinv", "svd", "--pinv_rcond", "0.01"])
	assert ns.pinv == "svd" and ns.pinv_rcond == 0.01
	assert parser.parse_args(common + ["--pinv_rcond", "0", "--pinv", "numpy"]).pinv_rcond == 0.0
	for bad in (["--pinv", "svd", "--pinv_rcond", "1"], ["--pinv", "svd", "--pinv_rcond", "-0.1"], ["--pinv", "numpy", "--pinv_rcond", "nan"],
				["--pinv", "svd", "--pinv_rcond", "small"], ["--pinv_rcond", "0.01"], ["--pinv", "auto", "--pinv_rcond", "0.01"],
				["--pinv", "device", "--pinv_rcond", "0.01"], ["--pinv_rcond", "0.01", "--pinv", "device32"], ["--pinv", "jacobi"]):
		with pytest.raises(SystemExit):
			parser.parse_args(common + bad)


def test_entry_point_B_arg_dict_rule_and_the_route_to_the_harness(tmp_path, monkeypatch):
	from anncur_amd import harness
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	common = COMMON_B + ["--res_dir", str(tmp_path)]
	parser = epB.build_parser()
	monkeypatch.setattr(epB, "run_eval_method", lambda *a, **kw: ({}, {}))
	cpu = torch.device("cpu")
	off = json.load(open(epB.run(parser.parse_args(common + ["--misc", "off"]), cpu)))
	svd = json.load(open(epB.run(parser.parse_args(common + ["--misc", "svd", "--pinv", "svd"]), cpu)))
	on = json.load(open(epB.run(parser.parse_args(common + ["--misc", "on", "--pinv", "svd", "--pinv_rcond", "0.01"]), cpu)))
	assert "pinv_rcond" not in off["other_args"] and off["other_args"]["pinv"] == "auto"
	assert "pinv_rcond" not in svd["other_args"] and svd["other_args"]["pinv"] == "svd"
	assert on["other_args"]["pinv"] == "svd" and on["other_args"]["pinv_rcond"] == 0.01
	assert {k: v for k, v in on["other_args"].items() if k not in ("pinv", "pinv_rcond", "misc")} == {k: v for k, v in off["other_args"].items() if k not in ("pinv", "misc")}
	monkeypatch.undo()
	seen = []
	monkeypatch.setattr(harness, "load_score_pickle", lambda f: {"ment_to_ent_scores": torch.zeros(3, 20), "ment_idxs": [0, 1, 2]})
	monkeypatch.setattr(harness, "to_device_matrix", lambda A, device, dtype: A)
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(kw) or {})
	for extra, want in (([], ("auto", None)), (["--pinv", "svd"], ("svd", None)), (["--pinv", "svd", "--pinv_rcond", "0.01"], ("svd", 0.01)),
						(["--pinv", "numpy", "--pinv_rcond", "0.5"], ("numpy", 0.5))):
		epB.run_eval_method("cur", "t.pkl", "r.pkl", parser.parse_args(common + extra), 0, cpu)
		kw = seen.pop()
		assert (kw["pinv_backend"], kw.get("pinv_rcond")) == want and ("pinv_rcond" in kw) == (want[1] is not None), (extra, kw)


def test_entry_point_A_arg_dict_rule_and_the_route_to_the_harness(tmp_path, monkeypatch):
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	seen = []
	monkeypatch.setattr(epA, "run", lambda **kw: seen.append(kw) or "res")
	common = COMMON_A + ["--res_dir", str(tmp_path)]
	for extra, want in (([], ("auto", None)), (["--pinv", "svd"], ("svd", None)), (["--pinv", "svd", "--pinv_rcond", "0.01"], ("svd", 0.01))):
		assert epA.main(common + extra) == "res"
		kw = seen.pop()
		assert (kw["pinv_backend"], kw.get("pinv_rcond")) == want and ("pinv_rcond" in kw) == (want[1] is not None)
		assert kw["arg_dict"]["pinv"] == want[0] and kw["arg_dict"].get("pinv_rcond") == want[1] and ("pinv_rcond" in kw["arg_dict"]) == (want[1] is not None)


def test_harness_passes_rcond_to_the_index_only_when_given(monkeypatch):
	"""run_entry_A -> run_approx_eval -> run_approx_eval_w_seed and run_eval_method_cur -> _sweep_adaptive_cells: the trailing pinv_rcond keyword
	reaches CURApprox / CURRowIndex as rcond=, and a default call makes exactly the constructor call it made before."""
	import inspect
	from anncur_amd import harness
	for fn in (harness.run_entry_A, harness.run_approx_eval, harness.run_approx_eval_w_seed, harness.run_eval_method_cur, harness._sweep_adaptive_cells):
		params = list(inspect.signature(fn).parameters.values())
		assert params[-1].name == "pinv_rcond" and params[-1].default is None, fn.__name__

	class Stop(Exception):
		pass

	seen = []

	def fake_index(*a, **kw):
		seen.append(kw)
		raise Stop

	monkeypatch.setattr(harness, "CURApprox", fake_index)
	monkeypatch.setattr(harness, "CURRowIndex", fake_index)
	monkeypatch.setattr(harness.ops, "gather_rows", lambda A, idx, **kw: A[np.asarray(idx)])
	monkeypatch.setattr(harness.ops, "gather_cols", lambda A, idx, **kw: A[:, np.asarray(idx)])
	monkeypatch.setattr(harness.ops, "rowwise_topk", lambda A, k, **kw: None)
	A = torch.zeros(6, 12)
	grids_a = {"eval_methods": ["cur"], "top_k_vals": [1], "top_k_retr_vals": [2], "n_ment_anchors_vals": [3], "n_ent_anchors_vals": [3]}
	grids_b = {"top_k_vals": [1], "top_k_retr_vals": [2], "n_ent_anchors_vals": [3]}
	for kw, want in (({}, None), ({"pinv_rcond": 0.01}, 0.01)):
		with pytest.raises(Stop):
			harness.run_entry_A(A, grids_a, 1, None, "svd", None, **kw)
		with pytest.raises(Stop):
			harness.run_eval_method_cur(A, A, 0, grids_b, pinv_backend="svd", **kw)
		with pytest.raises(Stop):
			harness._sweep_adaptive_cells(A, A, [0, 1, 2], None, [1], [2], 2, None, "svd", **kw)
		for got in seen:
			assert got["pinv_backend"] == "svd" and got.get("rcond") == want and ("rcond" in got) == (want is not None)
		assert len(seen) == 3
		del seen[:]
