"""Host side of the SoftMax item sampling: the numpy statement of the noise contract (tests/gumbel_numpy.py) against the known
answers of include/anncur_hip.h's formulas, every ValueError of ops.sample_topk and of AdaptiveSearcher's new arguments before any device
call, and the three flags of entry point B with their arg-dict rule.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_numpy as gn  # noqa: E402

# (seed, stream, row_key, item) -> (base, z, z >> 41, g)
KNOWN = [
	((0, 0, 0, 0), (0xe220a8397b1dcdaf, 0x48218226ff3cd4bf, 2363585, -0.23641102714856)),
	((1, 2, 3, 4), (0xf893a2eefb32555e, 0xb64447aaaeb323ca, 5972515, 1.07967356539464)),
	((2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31 - 1), (0xd3c3fc2c2de810ec, 0xaf24442f3a81cdf6, 5739042, 0.96868407755863)),
	((12345, 7, 100000, 99999), (0x6e7411b06820371c, 0xa0afdd8e4622e621, 5265390, 0.76417222328440)),
]


@pytest.mark.parametrize("point, want", KNOWN)
def test_numpy_statement_reproduces_the_known_answers(point, want):
	seed, stream, row_key, item = point
	base, z, top, g = want
	assert gn.base(seed, stream) == base
	assert gn.mix64(base ^ (row_key << 32 | item)) == z                                     # Python ints
	assert int(gn.counter(seed, stream, [row_key], [item])[0, 0]) == z                      # the array form
	assert int(gn.counter(seed, stream, np.array([row_key]).astype(np.uint32).view(np.int32), [item])[0, 0]) == z   # keys as the int32 the kernels are handed
	assert int(gn.bits23(seed, stream, [row_key], [item])[0, 0]) == top == z >> 41
	got = float(gn.gumbel64(seed, stream, [row_key], [item])[0, 0])
	assert abs(got - g) <= 1e-13
	assert abs(float(gn.bits_from_gumbel(got)) - top) <= 1e-6                                # the inverse the GPU test uses


def test_noise_range_and_numpy_draw_follows_the_softmax():
	"""u is strictly inside (0, 1), so g is finite, in [-2.82, 16.64]; and the statement itself draws from the softmax: the distribution
	test of tests/test_gpu_sample_topk.py on the host (chi-square 4.35 at 5 and 24.4 at 29 degrees of freedom on these inputs)."""
	for bits, lo, hi in ((0, -2.82, -2.81), (2 ** 23 - 1, 16.63, 16.64)):
		g = -np.log(-np.log((bits + 0.5) * 2.0 ** -23))
		assert lo <= g <= hi and np.isfinite(np.float32(g))
	scores = np.array([0, 1, 2, 3, -1, 0.5], dtype=np.float32)
	Q = 20000
	G = gn.gumbel64(0, 2, np.arange(Q), np.arange(6)).astype(np.float32)
	_, ids = gn.sample_reference(np.tile(scores, (Q, 1)), 1.0, G, 2)
	c1, c2 = gn.chi2_first_and_pairs(ids, scores)
	print(f"numpy draw: chi2 first = {c1:.2f} (5 dof), pairs = {c2:.2f} (29 dof)")
	assert c1 <= 20.5 and c2 <= 58.3


def test_sample_topk_value_errors_come_before_any_device_call():
	from anncur_amd import _lib, ops
	S = torch.zeros(3, 10)                                     # a CPU tensor: the device check would raise AnncurHipError
	for kw, msg in ((dict(temperature=0.0), r"finite temperature > 0"), (dict(temperature=-1.0), r"finite temperature > 0"),
					(dict(temperature=float("inf")), r"finite temperature > 0"), (dict(temperature=float("nan")), r"finite temperature > 0"),
					(dict(temperature=1e-40), r"1 / temperature = inf is not a finite fp32 number > 0"),
					(dict(temperature=1e60), r"1 / temperature = 0\.0 is not a finite fp32 number > 0"),
					(dict(seed=-1), r"seed = -1 outside \[0, 2\^64\)"), (dict(seed=2 ** 64), r"outside \[0, 2\^64\)"), (dict(seed=1.5), r"seed must be an integer"),
					(dict(stream=-1), r"stream = -1 outside \[0, 2\^32\)"), (dict(stream=2 ** 32), r"outside \[0, 2\^32\)"),
					(dict(row_keys=[0, 1]), r"one key per row: 3 \(got 2\)"), (dict(row_keys=torch.arange(4)), r"one key per row: 3 \(got 4\)")):
		with pytest.raises(ValueError, match=msg):
			ops.sample_topk(S, 2, **kw)
	for k in (0, 11, -1, 2.0):
		with pytest.raises(ValueError, match=r"outside 1\.\.min\(items, ANNCUR_MAX_TOPK\) = min\(10, 2048\) = 10"):
			ops.sample_topk(S, k)
	with pytest.raises(ValueError, match=rf"min\(5000, {_lib.MAX_TOPK}\) = {_lib.MAX_TOPK}"):
		ops.sample_topk(torch.zeros(1, 5000), _lib.MAX_TOPK + 1)
	with pytest.raises(ValueError, match="2-D"):
		ops.sample_topk(torch.zeros(10), 2)
	# the valid forms get as far as the device check: seed and stream at their ends, every row_keys form
	for kw in (dict(), dict(seed=2 ** 64 - 1, stream=2 ** 32 - 1), dict(temperature=0.25, row_keys=[5, 2 ** 32 - 1, 7]), dict(row_keys=np.arange(3)),
			   dict(row_keys=torch.tensor([1, 2, 3]))):
		with pytest.raises(_lib.AnncurHipError, match="no CPU fallback"):
			ops.sample_topk(S, 10, **kw)
	with pytest.raises(ValueError, match=r"temperature"):
		ops.sample_topk_dense(torch.zeros(3, 4), torch.zeros(10, 4), 2, temperature=0.0)
	with pytest.raises(ValueError, match=r"min\(10, 2048\) = 10"):
		ops.sample_topk_dense(torch.zeros(3, 4), torch.zeros(10, 4), 11)
	for kw, msg in ((dict(seed=-1), r"gumbel_noise: seed = -1"), (dict(stream=2 ** 32), r"gumbel_noise: stream"), (dict(I=0), r"I = 0 outside 1\.\.2\^31"),
					(dict(I=2 ** 31 + 1), r"outside 1\.\.2\^31"), (dict(rows=-1), r"rows = -1")):
		args = dict(seed=0, stream=0, rows=2, I=4)
		args.update(kw)
		with pytest.raises(ValueError, match=msg):
			ops.gumbel_noise(**args)
	# the bindings: both symbols with the header's argument counts
	assert len(_lib.SIGNATURES["anncur_sample_topk"][1]) == 15 and len(_lib.SIGNATURES["anncur_gumbel_noise"][1]) == 8
	lib = _lib.load()
	assert hasattr(lib, "anncur_sample_topk") and hasattr(lib, "anncur_gumbel_noise")


def test_library_refuses_bad_arguments_without_a_device():
	"""The C entry points check before they launch: ANNCUR_E_INVALID with the limit in the message, on a machine without a GPU too."""
	import ctypes
	from anncur_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(256)

	def call(Q=4, I=100, lds=100, inv_T=1.0, k=5, off=None, ids=None, n_sh=0, S=p):
		return lib.anncur_sample_topk(S, lds, Q, I, inv_T, 0, 0, None, off, ids, n_sh, k, p, p, None)
	for kw, msg in ((dict(k=0), b"1 <= k <= min(I, ANNCUR_MAX_TOPK) = min(100, 2048)"), (dict(k=101), b"min(100, 2048)"),
					(dict(I=5000, lds=5000, k=2049), b"min(5000, 2048)"), (dict(I=2 ** 31, lds=2 ** 31), b"I < 2^31"), (dict(I=0, lds=0), b"I < 2^31"),
					(dict(inv_T=0.0), b"finite and > 0"), (dict(inv_T=float("inf")), b"finite and > 0"), (dict(inv_T=float("nan")), b"finite and > 0"),
					(dict(inv_T=-1.0), b"finite and > 0"), (dict(lds=99), b"row pitch"), (dict(Q=-1), b"0 <= Q < 2^31"), (dict(n_sh=3), b"excl_ids is NULL"),
					(dict(n_sh=-1), b"[0, 2^31)"), (dict(S=None), b"null pointer")):
		assert call(**kw) == -1 and msg in lib.anncur_last_error(), (kw, lib.anncur_last_error())
	assert call(Q=0) == 0                                                                           # Q = 0: nothing to do
	assert lib.anncur_gumbel_noise(0, 0, None, 2, 0, p, 0, None) == -1 and b"1 <= I <= 2^31" in lib.anncur_last_error()
	assert lib.anncur_gumbel_noise(0, 0, None, 2, 2 ** 31 + 1, p, 2 ** 31 + 1, None) == -1
	assert lib.anncur_gumbel_noise(0, 0, None, 2, 8, p, 7, None) == -1 and b"row pitch" in lib.anncur_last_error()
	assert lib.anncur_gumbel_noise(0, 0, None, 0, 8, None, 8, None) == 0


def _index():
	from anncur_amd.cur import CURRowIndex
	index = CURRowIndex.__new__(CURRowIndex)
	index.R, index.m, index.col_idxs = torch.zeros(16, 5000), 5000, [2, 5, 700, 4999]
	return index


def test_searcher_strategy_arguments_are_checked_in_the_constructor():
	from anncur_amd.search import STRATEGIES, AdaptiveSearcher
	calls = []
	scorer = lambda q, i: calls.append(1)
	assert STRATEGIES == ("topk", "softmax")
	s = AdaptiveSearcher(_index(), scorer)
	assert (s.strategy, s.temperature, s.seed) == ("topk", 1.0, 0)
	s = AdaptiveSearcher(_index(), scorer, 0.5, True, "softmax", 0.25, 2 ** 64 - 1)               # the documented positional order
	assert (s.ridge, s.incremental, s.strategy, s.temperature, s.seed) == (0.5, True, "softmax", 0.25, 2 ** 64 - 1)
	with pytest.raises(ValueError, match=r"strategy = 'gumbel', need one of \('topk', 'softmax'\)"):
		AdaptiveSearcher(_index(), scorer, strategy="gumbel")
	for t in (0.0, -2.0, float("inf"), float("nan"), "1", None):
		with pytest.raises(ValueError, match=r"need a finite temperature > 0"):
			AdaptiveSearcher(_index(), scorer, strategy="softmax", temperature=t)
	for seed in (-1, 2 ** 64, 0.5, "3"):
		with pytest.raises(ValueError, match=r"AdaptiveSearcher: seed .*\[0, 2\^64\)"):
			AdaptiveSearcher(_index(), scorer, strategy="softmax", seed=seed)
	# the limits are the strategy's too, and still come before the first scorer call
	with pytest.raises(ValueError, match=r"above the limit of min\(items, ANNCUR_MAX_TOPK\)"):
		AdaptiveSearcher(_index(), scorer, strategy="softmax").search(np.arange(3), 5, 1100, 2)
	assert calls == []


def test_entry_point_B_flags_and_their_arg_dict_rule(tmp_path, monkeypatch):
	"""--adaptive_strategy / --adaptive_temperature / --adaptive_seed: at their defaults absent from the written other_args (the default run
	writes what it wrote before the flags existed); set, they reach harness.run_eval_method_cur together with --adaptive_rounds >= 2 only."""
	import json
	from anncur_amd import harness
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path), "--test_data_file", "t.pkl", "--train_data_file", "r.pkl"]
	parser = epB.build_parser()
	d = parser.parse_args(common)
	assert (d.adaptive_strategy, d.adaptive_temperature, d.adaptive_seed) == ("topk", 1.0, 0)
	a = parser.parse_args(common + ["--adaptive_strategy", "softmax", "--adaptive_temperature", "0.5", "--adaptive_seed", str(2 ** 64 - 1)])
	assert (a.adaptive_strategy, a.adaptive_temperature, a.adaptive_seed) == ("softmax", 0.5, 2 ** 64 - 1)
	for bad in (["--adaptive_strategy", "gumbel"], ["--adaptive_temperature", "0"], ["--adaptive_temperature", "inf"], ["--adaptive_temperature", "nan"],
				["--adaptive_seed", "-1"], ["--adaptive_seed", str(2 ** 64)]):
		with pytest.raises(SystemExit):
			parser.parse_args(common + bad)
	assert harness.ADAPTIVE_SOFTMAX_PREFIX == "exact_vs_reranked_adaptive_softmax_retvr" and harness.ADAPTIVE_PREFIX == "exact_vs_reranked_adaptive_retvr"
	# the arg_dict rule, with the evaluation itself stubbed out
	monkeypatch.setattr(epB, "run_eval_method", lambda *a, **kw: ({}, {}))
	cpu = torch.device("cpu")
	new = ("adaptive_strategy", "adaptive_temperature", "adaptive_seed")
	off = json.load(open(epB.run(parser.parse_args(common + ["--misc", "off", "--adaptive_rounds", "2"]), cpu)))
	dflt = json.load(open(epB.run(parser.parse_args(common + ["--misc", "dflt", "--adaptive_rounds", "2", "--adaptive_strategy", "topk", "--adaptive_temperature", "1",
																 "--adaptive_seed", "0"]), cpu)))
	on = json.load(open(epB.run(parser.parse_args(common + ["--misc", "on", "--adaptive_rounds", "2", "--adaptive_strategy", "softmax", "--adaptive_temperature", "2.5",
															   "--adaptive_seed", "7"]), cpu)))
	assert not any(key in off["other_args"] for key in new) and not any(key in dflt["other_args"] for key in new)
	assert open(f"{tmp_path}/method=cur_dflt.json").read().replace('"misc": "dflt"', '"misc": "off"') == open(f"{tmp_path}/method=cur_off.json").read()
	assert [on["other_args"][key] for key in new] == ["softmax", 2.5, 7]
	assert {k: v for k, v in on["other_args"].items() if k not in new + ("misc",)} == {k: v for k, v in off["other_args"].items() if k != "misc"}
	only_t = json.load(open(epB.run(parser.parse_args(common + ["--misc", "t", "--adaptive_temperature", "3"]), cpu)))
	assert only_t["other_args"]["adaptive_temperature"] == 3.0 and "adaptive_strategy" not in only_t["other_args"] and "adaptive_seed" not in only_t["other_args"]
	# the route to the harness, with the harness call and the loading stubbed out
	monkeypatch.undo()
	seen = []
	monkeypatch.setattr(harness, "load_score_pickle", lambda f: {"ment_to_ent_scores": torch.zeros(3, 20), "ment_idxs": [0, 1, 2]})
	monkeypatch.setattr(harness, "to_device_matrix", lambda A, device, dtype: A)
	monkeypatch.setattr(harness, "run_eval_method_cur", lambda *a, **kw: seen.append(kw) or {})
	soft = ["--adaptive_strategy", "softmax", "--adaptive_temperature", "0.5", "--adaptive_seed", "9"]
	for extra, want in (([], {}), (soft, {}), (["--adaptive_rounds", "3"], {"adaptive_rounds": 3}),
						(["--adaptive_rounds", "3", "--adaptive_strategy", "softmax"], {"adaptive_rounds": 3, "adaptive_strategy": "softmax"}),
						(["--adaptive_rounds", "3"] + soft, {"adaptive_rounds": 3, "adaptive_strategy": "softmax", "adaptive_temperature": 0.5, "adaptive_seed": 9}),
						(["--adaptive_rounds", "2", "--adaptive_incremental"] + soft,
						 {"adaptive_rounds": 2, "adaptive_incremental": True, "adaptive_strategy": "softmax", "adaptive_temperature": 0.5, "adaptive_seed": 9})):
		epB.run_eval_method("cur", "t.pkl", "r.pkl", parser.parse_args(common + extra), 0, cpu)
		kw = seen.pop()
		assert {k: v for k, v in kw.items() if k.startswith("adaptive_")} == want, (extra, kw)
