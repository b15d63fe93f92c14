"""Host side of the pivoted anchor selection: the library exports the new calls and refuses what is outside their limits
without a device, the numpy restatement (tests/pivot_numpy.py) equals LAPACK's dgeqp3 pivots and the closed form of the Hadamard data,
AnchorSelection's errors, and --anchor_selection of entry point B with its arg-dict rule.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pivot_numpy as pn  # noqa: E402


def test_library_exports_the_selection_and_its_workspace_query():
	from anncur_amd import _lib
	lib = _lib.load()
	for name, n_args in (("anncur_select_pivoted", 12), ("anncur_select_pivoted_workspace_bytes", 3), ("anncur_select_pivoted_slice_items", 1)):
		assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
	assert lib.anncur_select_pivoted_slice_items(_lib.F32) * 4 == lib.anncur_select_pivoted_slice_items(_lib.BF16) * 2 > 0   # 16 bytes per thread
	assert lib.anncur_select_pivoted_slice_items(7) == 0


def test_workspace_query_is_zero_outside_the_limits():
	from anncur_amd import _lib
	ws = _lib.load().anncur_select_pivoted_workspace_bytes
	for m, kq, k in ((100, 10, 0), (100, 10, 11), (5, 10, 6), (5000, 4096, _lib.MAX_TOPK + 1), (100, 0, 1), (100, _lib.LSTSQ_MAX_KQ + 1, 1), (2 ** 31, 10, 1),
					 (0, 10, 1), (-1, 10, 1), (100, -1, 1), (100, 10, -1)):
		assert ws(m, kq, k) == 0, (m, kq, k)
	# inside: the header, d[m], the basis [k x kq] and the per-workgroup maxima, each a multiple of 256 bytes
	for m, kq, k in ((100, 10, 10), (1, 1, 1), (5000, 4096, _lib.MAX_TOPK), (2 ** 31 - 1, 1, 1)):
		got = ws(m, kq, k)
		assert got % 256 == 0 and got >= 8 * m + 8 * k * kq + 256, (m, kq, k, got)


def test_library_refuses_bad_arguments_without_a_device():
	from anncur_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(256)

	def call(dtype=0, ldr=100, kq=10, m=100, k=5, R=p, ids=p, gain=p, n_sel=p, ws=p, ws_bytes=1 << 40):
		return lib.anncur_select_pivoted(R, dtype, ldr, kq, m, k, ids, gain, n_sel, ws, ws_bytes, None)
	for kw, msg in ((dict(k=0), b"1 <= k <= min(kq, m, ANNCUR_MAX_TOPK) = min(10, 100, 2048)"), (dict(k=11), b"min(10, 100, 2048)"), (dict(m=4, ldr=4), b"min(10, 4, 2048)"),
					(dict(kq=4096, m=5000, ldr=5000, k=2049), b"min(4096, 5000, 2048)"), (dict(kq=0), b"1 <= kq <= 4096"), (dict(kq=4097), b"1 <= kq <= 4096"),
					(dict(m=2 ** 31, ldr=2 ** 31), b"m < 2^31"), (dict(dtype=2), b"ANNCUR_F32 or ANNCUR_BF16"), (dict(ldr=99), b"row pitch"),
					(dict(R=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(gain=None), b"null pointer"), (dict(n_sel=None), b"null pointer")):
		assert call(**kw) == -1 and msg in lib.anncur_last_error(), (kw, lib.anncur_last_error())
	for kw in (dict(ws=None), dict(ws_bytes=lib.anncur_select_pivoted_workspace_bytes(100, 10, 5) - 1), dict(ws=ctypes.c_void_p(264))):
		assert call(**kw) == -2 and b"workspace missing, misaligned (256 bytes) or too small" in lib.anncur_last_error(), kw


def test_select_pivoted_value_errors_come_before_any_device_call():
	from anncur_amd import _lib, ops
	R = torch.zeros(10, 100)                                   # a CPU tensor: the device check would raise AnncurHipError
	for k in (0, 11, -1):
		with pytest.raises(ValueError, match=r"outside 1\.\.min\(kq, items, ANNCUR_MAX_TOPK\) = min\(10, 100, 2048\) = 10"):
			ops.select_pivoted(R, k)
	with pytest.raises(ValueError, match="k must be an integer"):
		ops.select_pivoted(R, 2.0)
	with pytest.raises(ValueError, match=r"kq = 4097 anchor queries, outside 1\.\.ANNCUR_LSTSQ_MAX_KQ"):
		ops.select_pivoted(torch.zeros(4097, 1), 1)
	with pytest.raises(ValueError, match="2-D"):
		ops.select_pivoted(torch.zeros(10), 1)
	with pytest.raises(_lib.AnncurHipError, match="no CPU fallback"):
		ops.select_pivoted(R, 10)


@pytest.mark.parametrize("kq, m, k, rank, noise, seed", pn.GENERIC)
def test_restatement_equals_lapack_pivots(kq, m, k, rank, noise, seed):
	"""scipy.linalg.qr(pivoting=True) is dgeqp3: the same greedy rule with downdated norms.  Equality needs the argmax of every step to be
	clear of ties, which the gap says: the GPU test asks 2^-30 of it, these inputs give 1e-5 or more."""
	from scipy.linalg import qr
	R = pn.low_rank(kq, m, rank, noise, seed)
	ids, gains, n_sel, gaps = pn.select(R, k)
	print(f"{kq} x {m}, k = {k}: minimum gap {gaps.min():.3g}")
	assert n_sel == k and gaps.min() >= 2.0 ** -30
	_, rr, piv = qr(R.astype(np.float64), mode="economic", pivoting=True)
	assert np.array_equal(ids, piv[:k])
	assert np.allclose(gains, np.diag(rr)[:k] ** 2, rtol=1e-10, atol=0.0)         # |r_tt|^2 = the residual norm the pivot had
	assert (np.diff(gains) <= 2.0 ** -40 * gains[0]).all()
	# nested: the call with k' < k is a prefix
	ids2, gains2, n2, _ = pn.select(R, k // 2)
	assert n2 == k // 2 and np.array_equal(ids2, ids[:k // 2]) and np.array_equal(gains2, gains[:k // 2])


def test_restatement_equals_the_closed_form_on_hadamard_data():
	rng = np.random.default_rng(5)
	scales = rng.integers(1, 10, 323)                           # 9 values on 64 directions: many exact ties
	scales[rng.choice(323, 40, replace=False)] *= -1
	want = pn.hadamard_closed_form(scales, 80)
	ids, gains, n_sel, _ = pn.select(pn.hadamard_items(scales, 96), 80)          # kq = 96: k = 80 above the rank, inside k <= kq
	assert n_sel == want[2] == 64 and np.array_equal(ids, want[0]) and np.array_equal(gains, want[1])
	assert (ids[64:] == -1).all() and (gains[64:] == 0.0).all()
	assert len(set(gains[:64].tolist())) < 64 and len(set(gains[:64].tolist())) > 1                     # ties, and not only ties
	# a rank below 64: directions 40.. hold zeros only; and columns of NaN / inf are never taken
	scales[np.arange(323) % 64 >= 40] = 0
	R = pn.hadamard_items(scales, 96).astype(np.float64)
	R[:, 3], R[5, 70] = np.nan, np.inf
	want = pn.hadamard_closed_form(scales, 80, never=(3, 70))
	ids, gains, n_sel, _ = pn.select(R, 80)
	assert n_sel == want[2] == 40 and np.array_equal(ids, want[0]) and np.array_equal(gains, want[1])


@pytest.mark.parametrize("n, kq, m, k", [(16, 16, 1300, 24), (256, 256, 1500, 40), (256, 600, 1777, 32), (1024, 1027, 2100, 24)])
def test_restatement_equals_the_closed_form_at_other_hadamard_orders(n, kq, m, k):
	"""The closed form with the Hadamard order as a parameter (the data of tests/test_gpu_select_pivoted_large.py), against the restatement:
	ids, gains and n_sel are equal.  kq > n appends zero rows; with n = 16 the rank stops the k = 24 picks at 16."""
	rng = np.random.default_rng(n + kq)
	scales = rng.integers(1, 10, m)
	scales[rng.choice(m, m // 8, replace=False)] *= -1
	want = pn.hadamard_closed_form(scales, k, n=n)
	ids, gains, n_sel, _ = pn.select(pn.hadamard_items(scales, kq, n=n), k)
	assert n_sel == want[2] == min(k, n) and np.array_equal(ids, want[0]) and np.array_equal(gains, want[1])
	assert np.array_equal(gains[:n_sel], float(n) * scales[ids[:n_sel]].astype(np.float64) ** 2) and (ids[n_sel:] == -1).all()
	# NaN columns among the would-be winners are passed over, here as there
	never = tuple(int(i) for i in want[0][:3])
	R = pn.hadamard_items(scales, kq, n=n).astype(np.float64)
	R[:, list(never)] = np.nan
	want = pn.hadamard_closed_form(scales, k, never=never, n=n)
	ids, gains, n_sel, _ = pn.select(R, k)
	assert n_sel == want[2] and np.array_equal(ids, want[0]) and np.array_equal(gains, want[1]) and not np.isin(never, ids).any()


def test_hadamard_order_must_be_a_power_of_4():
	for n in (2, 8, 32, 48, 128, 512):
		with pytest.raises(AssertionError):
			pn.hadamard_items(np.ones(10, dtype=np.int64), 1024, n=n)
		with pytest.raises(AssertionError):
			pn.hadamard_closed_form(np.ones(10, dtype=np.int64), 4, n=n)
	for n in (1, 4, 16, 64, 256, 1024, 4096):
		assert pn._power_of_4(n)


def test_anchor_selection_sorted_and_its_errors():
	from anncur_amd.cur import ANCHOR_SELECTIONS, AnchorSelection, select_anchor_items
	assert ANCHOR_SELECTIONS == ("random", "pivoted")
	sel = AnchorSelection(np.array([7, 2, 9, 4], dtype=np.int32), [4.0, 3.0, 2.0, 1.0])
	assert sel.n_sel == 4 and sel.order.dtype == np.int64 and sel.gains.dtype == np.float64
	assert sel.sorted(0) == [] and sel.sorted(2) == [2, 7] and sel.sorted(4) == sel.sorted() == [2, 4, 7, 9]
	assert all(type(i) is int for i in sel.sorted(4))
	with pytest.raises(ValueError, match=r"n = 5 anchor items asked of a selection of n_sel = 4"):
		sel.sorted(5)
	for bad in (-1, 1.5, True):
		with pytest.raises(ValueError, match="integer >= 0"):
			sel.sorted(bad)
	# "random" is the harness' _select on the caller's generator
	rows = torch.zeros(3, 50)
	got = select_anchor_items(rows, 8, method="random", rng=np.random.default_rng(4))
	assert got.gains is None and got.sorted(8) == sorted(int(i) for i in np.random.default_rng(4).choice(50, size=8, replace=False)) == list(got.order)
	with pytest.raises(ValueError, match="needs rng="):
		select_anchor_items(rows, 8, method="random")
	with pytest.raises(ValueError, match="takes no rng"):
		select_anchor_items(rows, 8, method="pivoted", rng=np.random.default_rng(0))
	with pytest.raises(ValueError, match=r"method = 'qr', need one of \('random', 'pivoted'\)"):
		select_anchor_items(rows, 8, method="qr")


def test_harness_refuses_an_unknown_anchor_selection():
	from anncur_amd import harness
	with pytest.raises(ValueError, match=r"anchor_selection = qr not supported \(one of random, pivoted\)"):
		harness.run_eval_method_cur(torch.zeros(2, 5), torch.zeros(2, 5), 0, {"top_k_vals": [1], "top_k_retr_vals": [2], "n_ent_anchors_vals": [1]}, anchor_selection="qr")


def test_entry_point_B_flag_and_its_arg_dict_rule(tmp_path, monkeypatch):
	"""--anchor_selection: random by default and then absent from the written other_args (the default run writes what it wrote before the flag
	existed); pivoted is recorded, reaches harness.run_eval_method_cur for method cur only, and is an argparse error with --n_seeds > 1."""
	from anncur_amd import harness
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path), "--test_data_file", "t.pkl", "--train_data_file", "r.pkl"]
	parser = epB.build_parser()
	assert parser.parse_args(common).anchor_selection == "random"
	assert parser.parse_args(common + ["--anchor_selection", "pivoted"]).anchor_selection == "pivoted"
	assert parser.parse_args(common + ["--anchor_selection", "random", "--n_seeds", "3"]).n_seeds == 3
	for bad in (["--anchor_selection", "qr"], ["--anchor_selection", "pivoted", "--n_seeds", "2"], ["--n_seeds", "2", "--anchor_selection", "pivoted"]):
		with pytest.raises(SystemExit):
			parser.parse_args(common + bad)
	monkeypatch.setattr(epB, "run_eval_method", lambda *a, **kw: ({}, {}))
	cpu = torch.device("cpu")
	off = json.load(open(epB.run(parser.parse_args(common + ["--misc", "off"]), cpu)))
	dflt = json.load(open(epB.run(parser.parse_args(common + ["--misc", "dflt", "--anchor_selection", "random"]), cpu)))
	on = json.load(open(epB.run(parser.parse_args(common + ["--misc", "on", "--anchor_selection", "pivoted"]), cpu)))
	assert "anchor_selection" not in off["other_args"] and "anchor_selection" not in dflt["other_args"]
	assert open(f"{tmp_path}/method=cur_dflt.json").read().replace('"misc": "dflt"', '"misc": "off"') == open(f"{tmp_path}/method=cur_off.json").read()
	assert on["other_args"]["anchor_selection"] == "pivoted"
	assert {k: v for k, v in on["other_args"].items() if k not in ("anchor_selection", "misc")} == {k: v for k, v in off["other_args"].items() if k != "misc"}
	# the route to the harness, with the harness call and the loading stubbed out
	monkeypatch.undo()
	seen = []
	monkeypatch.setattr(harness, "load_score_pickle", lambda f: {"ment_to_ent_scores": torch.zeros(3, 20), "ment_idxs": [0, 1, 2]})
	monkeypatch.setattr(harness, "to_device_matrix", lambda A, device, dtype: A)
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(kw) or {})
	for extra, want in (([], {}), (["--anchor_selection", "random"], {}), (["--anchor_selection", "pivoted"], {"anchor_selection": "pivoted"}),
						(["--anchor_selection", "pivoted", "--adaptive_rounds", "2"], {"anchor_selection": "pivoted", "adaptive_rounds": 2})):
		epB.run_eval_method("cur", "t.pkl", "r.pkl", parser.parse_args(common + extra), 0, cpu)
		kw = seen.pop()
		assert {k: v for k, v in kw.items() if k in ("anchor_selection", "adaptive_rounds")} == want, (extra, kw)
