"""Host side of the incremental per-query solve: the limits of ops.LstsqState and of adaptive_limits(incremental=True), each a
ValueError that names the limit and is raised before any launch; the state size and the limits of the C entry points, which answer
without a device.  No GPU needed."""
import ctypes
import re

import pytest
import torch


def _state(kq=100, Q=3, cap=48, **kw):
	from anncur_amd import ops
	return ops.LstsqState(torch.zeros(10, kq), Q, cap, **kw)


def _rows(Q, n, ids_dtype=torch.int32, c_dtype=torch.float32):
	return torch.zeros((Q, n), dtype=ids_dtype), torch.zeros((Q, n), dtype=c_dtype)


def test_state_limits_name_the_constant():
	from anncur_amd import _lib, ops
	assert ops.LSTSQ_STATE_LIMIT_BYTES == 32 << 30
	for cap in (0, -1, 513):
		with pytest.raises(ValueError, match=rf"cap = {cap} scored items per query, outside 1\.\.ANNCUR_LSTSQ_MAX_G = 512"):
			_state(cap=cap)
	with pytest.raises(ValueError, match=r"kq = 4097 anchor queries, outside 1\.\.ANNCUR_LSTSQ_MAX_KQ = 4096"):
		_state(kq=4097)
	with pytest.raises(ValueError, match="need ridge >= 0"):
		_state(ridge=-0.5)
	with pytest.raises(ValueError, match="Rt must be a float32 tensor"):
		ops.LstsqState(torch.zeros(10, 4, dtype=torch.float64), 3, 4)
	# the byte cap: the message names the remedy
	need = ops.lstsq_state_bytes(3, 48)
	assert need > 0
	with pytest.raises(ValueError, match=rf"3 queries at cap = 48 need {need} bytes of state, above max_bytes = {need - 1}: search the queries in batches"):
		_state(max_bytes=need - 1)
	assert _state(max_bytes=need).nbytes == need
	# cfg2's 10 000 queries at cap = 456 fit under the default, 20 000 do not
	assert 17e9 < ops.lstsq_state_bytes(10 ** 4, 456) < 17.5e9
	with pytest.raises(ValueError, match="search the queries in batches"):
		ops.LstsqState(torch.zeros(10, 500), 2 * 10 ** 4, 456)
	s = _state()
	assert (s.n, s.cap, s.kq, s.Q, s.ridge) == (0, 48, 100, 3, 0.0) and s._buf is None     # nothing is allocated before the first extend


def test_extend_limits_are_raised_before_any_launch():
	from anncur_amd import _lib
	s = _state(kq=40, Q=3, cap=48)
	shape = r"ids int32 and C float32, both \[Q x n\] of one shape with Q = 3"
	for ids, C in (_rows(3, 8, ids_dtype=torch.int64), _rows(3, 8, c_dtype=torch.float64), _rows(2, 8), (torch.zeros((3, 8), dtype=torch.int32), torch.zeros(3, 9)),
				   (torch.zeros(8, dtype=torch.int32), torch.zeros(8))):
		with pytest.raises(ValueError, match=shape):
			s.extend(ids, C)
	with pytest.raises(ValueError, match=r"rows of 0 positions, but 0 are absorbed already"):
		s.extend(*_rows(3, 0))
	with pytest.raises(ValueError, match=r"rows of 49 positions, above this state's cap = 48"):
		s.extend(*_rows(3, 49))
	with pytest.raises(ValueError, match=r"rows of 41 positions, above kq = 40 anchor queries: the query side has no incremental form \(lstsq_rows solves it\)"):
		s.extend(*_rows(3, 41))
	s.n = 16       # as after a call that absorbed 16 positions
	for n in (16, 12):
		with pytest.raises(ValueError, match=rf"rows of {n} positions, but 16 are absorbed already"):
			s.extend(*_rows(3, n))
	with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):     # every host check passed: there is no CPU path
		s.extend(*_rows(3, 17))
	assert s.n == 16 and s._buf is None


def test_c_entry_points_answer_size_and_limits_without_a_device():
	from anncur_amd import _lib
	lib = _lib.load()
	sb = lib.anncur_lstsq_state_bytes
	assert sb(1, 0) == 0 and sb(1, 513) == 0 and sb(1, -3) == 0 and sb(-1, 16) == 0 and sb(0, 16) == 0
	assert sb(1, 1) > 0 and sb(1, 512) > 0
	sizes = [sb(1, cap) for cap in range(1, 513)]
	assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] == sizes[15] < sizes[16]      # monotone in cap, in steps of the 16-pitch
	for cap in (1, 16, 17, 456, 512):
		capp = -(-cap // 16) * 16
		assert sb(1, cap) >= ((capp + 2) * capp + 3) * 8                                            # G / L, z, y and a three-word header at least
		assert sb(7, cap) == 7 * sb(1, cap)
	assert sb(10 ** 4, 512) == 10 ** 4 * sb(1, 512) > 2 ** 32                                       # (size_t)
	null = ctypes.c_void_p(None)

	def extend(kq, n_old, n_new, cap, ridge=0.0, Q=1):
		return lib.anncur_lstsq_extend(null, kq, 10, kq, null, n_new, null, n_new, Q, n_old, n_new, cap, ridge, null, kq, null, null, 0, null)
	for args, msg in (((16, 0, 17, 32), r"n_new = 17 scored items above kq = 16: the query side has no incremental form"),
					  ((64, 0, 33, 32), r"0 <= n_old < n_new <= cap"), ((64, 8, 8, 32), r"0 <= n_old < n_new <= cap"), ((64, -1, 8, 32), r"0 <= n_old < n_new <= cap"),
					  ((64, 0, 8, 513), r"1 <= cap <= 512"), ((64, 0, 8, 0), r"1 <= cap <= 512"), ((5000, 0, 8, 16), r"1 <= kq <= 4096")):
		assert extend(*args) == -1 and re.search(msg, lib.anncur_last_error().decode())             # ANNCUR_E_INVALID before any pointer is read
	assert extend(64, 0, 8, 32, ridge=-1.0) == -1 and b"ridge >= 0" in lib.anncur_last_error()
	assert extend(64, 0, 8, 32, Q=0) == 0                                                           # Q = 0: nothing to do
	ms = (ctypes.c_float * 3)()
	assert lib.anncur_lstsq_extend_timed(null, 64, 10, 64, null, 8, null, 8, 0, 0, 8, 32, 0.0, null, 64, null, null, 0, null, ms) == 0
	assert lib.anncur_lstsq_extend_timed(null, 64, 10, 64, null, 8, null, 8, 0, 0, 8, 32, 0.0, null, 64, null, null, 0, null, None) == -1


def test_adaptive_limits_incremental_needs_the_item_side():
	from anncur_amd.search import adaptive_limits
	# kc + (n_rounds - 1) k_step = 24 + 3 * 12 = 60 against kq
	assert adaptive_limits(24, 60, 6000, 10, 12, 4, incremental=True) is None
	with pytest.raises(ValueError, match=r"incremental=True keeps a per-query factorisation of kc \+ \(n_rounds - 1\) \* k_step = 24 \+ 3 \* 12 = 60 scored items, "
										 r"above kq = 59 anchor queries.*use incremental=False"):
		adaptive_limits(24, 59, 6000, 10, 12, 4, incremental=True)
	assert adaptive_limits(24, 59, 6000, 10, 12, 4) is None and adaptive_limits(24, 59, 6000, 10, 12, 4, False) is None      # the default: today's limits
	assert adaptive_limits(24, 16, 6000, 10, 500, 1, incremental=True) is None                                               # one round builds no state
	with pytest.raises(ValueError, match=r"above ANNCUR_LSTSQ_MAX_G = 512"):                                                 # (the limit on g comes first)
		adaptive_limits(4, 1000, 5000, 5, 600, 2, incremental=True)


def test_searcher_takes_the_switch_and_checks_before_the_first_scorer_call():
	import numpy as np
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher
	index = CURRowIndex.__new__(CURRowIndex)
	index.R, index.m, index.col_idxs = torch.zeros(16, 5000), 5000, [2, 5, 700, 4999]
	calls = []
	scorer = lambda q, i: calls.append(1)
	assert AdaptiveSearcher(index, scorer).incremental is False
	s = AdaptiveSearcher(index, scorer, ridge=0.5, incremental=True)
	assert s.incremental is True and s.ridge == 0.5
	with pytest.raises(ValueError, match=r"4 \+ 2 \* 10 = 24 scored items, above kq = 16"):
		s.search(np.arange(3), 5, 10, 3)
	assert calls == []


def test_entry_point_B_flag_and_its_arg_dict_rule(tmp_path, monkeypatch):
	"""--adaptive_incremental: off by default and then absent from the written other_args (the default run writes what it wrote before the flag
	existed); on, it reaches harness.run_eval_method_cur together with --adaptive_rounds >= 2 only."""
	import json
	from anncur_amd import harness
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path), "--test_data_file", "t.pkl", "--train_data_file", "r.pkl"]
	parser = epB.build_parser()
	assert parser.parse_args(common).adaptive_incremental is False
	assert parser.parse_args(common + ["--adaptive_incremental"]).adaptive_incremental is True
	# the arg_dict rule, with the evaluation itself stubbed out
	monkeypatch.setattr(epB, "run_eval_method", lambda *a, **kw: ({}, {}))
	cpu = torch.device("cpu")
	off = json.load(open(epB.run(parser.parse_args(common + ["--misc", "off", "--adaptive_rounds", "2"]), cpu)))
	on = json.load(open(epB.run(parser.parse_args(common + ["--misc", "on", "--adaptive_rounds", "2", "--adaptive_incremental"]), cpu)))
	assert "adaptive_incremental" not in off["other_args"] and on["other_args"]["adaptive_incremental"] is True
	assert {k: v for k, v in on["other_args"].items() if k not in ("adaptive_incremental", "misc")} == {k: v for k, v in off["other_args"].items() if k != "misc"}
	# the route to the harness, with the harness call and the loading stubbed out
	monkeypatch.undo()
	seen = []
	monkeypatch.setattr(harness, "load_score_pickle", lambda f: {"ment_to_ent_scores": torch.zeros(3, 20), "ment_idxs": [0, 1, 2]})
	monkeypatch.setattr(harness, "to_device_matrix", lambda A, device, dtype: A)
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(kw) or {})
	for extra, want in (([], None), (["--adaptive_incremental"], None), (["--adaptive_rounds", "3"], (3, None)),
						(["--adaptive_rounds", "3", "--adaptive_incremental"], (3, True))):
		epB.run_eval_method("cur", "t.pkl", "r.pkl", parser.parse_args(common + extra), 0, cpu)
		kw = seen.pop()
		assert (kw.get("adaptive_rounds"), kw.get("adaptive_incremental")) == (want or (None, None)), (extra, kw)
