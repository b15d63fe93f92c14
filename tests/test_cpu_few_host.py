"""Host side of the small-batch route (no GPU): the numpy model of its select (tests/few_numpy.py) against topk_ref, the host
validation of ops.score_topk_few / score_rows_few, the plan and the support query at their boundaries, the C ABI's new symbols."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import few_numpy as fn  # noqa: E402
from topk_numpy import topk_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"anncur_score_topk_few_supported": 4, "anncur_score_topk_few_workspace_bytes": 4, "anncur_score_topk_few": 13,
			   "anncur_score_rows_few": 12, "anncur_score_topk_few_plan": 6}


def _same(got, want):
	assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ the model of launch 2
@pytest.mark.parametrize("I,k", [(1, 1), (63, 63), (64, 5), (65, 65), (4101, 100), (16421, 100), (16421, 1), (16421, 128), (16421, 129), (70001, 1024)])
def test_model_equals_topk_ref_on_random_rows(I, k):
	rng = np.random.default_rng(I + k)
	row = rng.standard_normal(I).astype(np.float32)
	val, ids, st = fn.select_model(row, k)
	_same((val, ids), topk_ref(row, k))
	G = -(-I // 64)
	assert st["fallback"] == 0 and st["n_cand"] <= fn.cand_cap(k)
	if G < k:     # fewer group maxima than k: no threshold, every group is read and every item is a candidate
		assert st["tau"] == -np.inf and st["groups_read"] == G and st["n_cand"] == I
	else:         # k groups reach tau, and at least k items
		assert k <= st["groups_read"] <= G and k <= st["n_cand"] < I or I == k


def test_model_on_tie_heavy_rows_keeps_the_smaller_id():
	rng = np.random.default_rng(7)
	row = rng.integers(-3, 4, 16421).astype(np.float32)      # seven values: thousands of ties at the threshold
	for k in (1, 100, 1024):
		val, ids, st = fn.select_model(row, k)
		_same((val, ids), topk_ref(row, k))
		assert (np.diff(ids[val == val[0]]) > 0).all()
	# k = 100: tau = 3 (257 groups, nearly all hold a 3), about 16421 / 7 candidates: under the cap
	_, _, st = fn.select_model(row, 100)
	assert st["tau"] == 3 and st["fallback"] == 0 and st["n_cand"] == int((row >= 3).sum())


def test_model_falls_back_when_every_score_ties():
	row = np.full(20000, 5.0, dtype=np.float32)
	for k in (1, 100, 2048):
		val, ids, st = fn.select_model(row, k)
		_same((val, ids), topk_ref(row, k))
		assert np.array_equal(ids, np.arange(k)) and st["fallback"] == 1
		assert st["groups_read"] == 313 and st["n_cand"] == 20000      # one round of 1024 maxima covers the row


def test_model_stops_the_walk_at_the_round_that_overflows():
	row = np.full(1024 * 64 * 3, 1.0, dtype=np.float32)
	_, ids, st = fn.select_model(row, 10)
	assert st["fallback"] == 1 and st["groups_read"] == 1024 and st["n_cand"] == 65536 and np.array_equal(ids, np.arange(10))


def test_model_with_nan_blocks_and_infinities():
	rng = np.random.default_rng(3)
	row = rng.standard_normal(4101).astype(np.float32)
	row[0], row[4100], row[700:900] = np.nan, np.nan, np.nan      # item 0, item I - 1, three whole groups and two partial ones
	row[5], row[4000] = np.inf, -np.inf
	for k in (1, 64, 100):
		val, ids, st = fn.select_model(row, k)
		_same((val, ids), topk_ref(row, k))
		assert ids[0] == 5 and not np.isin(ids, [0, 4100]).any() and st["fallback"] == 0
	gm = fn.group_maxima(row)[0]
	assert np.isnan(gm[11:14]).all() and not np.isnan(gm[[10, 14]]).any() and gm[0] == np.inf
	# fewer than k non-NaN scores: all of them, then pads
	short = np.full(300, np.nan, dtype=np.float32)
	short[[3, 100, 299]] = [1.0, -np.inf, 2.0]
	val, ids, st = fn.select_model(short, 10)
	_same((val, ids), topk_ref(short, 10))
	assert ids.tolist() == [299, 3, 100] + [-1] * 7 and st["n_cand"] == 3 and st["groups_read"] == 3
	# a row of NaN: k pads, nothing read
	val, ids, st = fn.select_model(np.full(500, np.nan, dtype=np.float32), 4)
	assert ids.tolist() == [-1] * 4 and np.isneginf(val).all() and st["groups_read"] == 0 and st["n_cand"] == 0


def test_cand_cap_follows_the_selector_classes():
	assert [fn.cand_cap(k) for k in (1, 128, 129, 512, 513, 2048)] == [4352, 4352, 5120, 5120, 8192, 8192]


# ------------------------------------------------------------------ ops: validation before any device
def _operands(Q, I, Kp, ldx=None):
	ldx = ldx or Kp
	X = torch.zeros((Q, ldx), dtype=torch.bfloat16)[:, :Kp]
	return X, torch.zeros((-(-I // 32) * 32, Kp), dtype=torch.bfloat16)


def test_score_topk_few_validates_on_the_host():
	from anncur_amd import _lib, ops
	X, E = _operands(65, 1000, 64)
	with pytest.raises(ValueError, match=r"Q = 65 .*1\.\.64"):
		ops.score_topk_few(X, E, 1000, 10)
	X, E = _operands(4, 1000, 64)
	with pytest.raises(ValueError, match=r"k = 1001 .*min\(1000, 2048\) = 1000"):
		ops.score_topk_few(X, E, 1000, 1001)
	with pytest.raises(ValueError, match=r"k = 0 "):
		ops.score_topk_few(X, E, 1000, 0)
	X, E = _operands(4, 5000, 64)
	with pytest.raises(ValueError, match=r"k = 2049 .*= 2048"):
		ops.score_topk_few(X, E, 5000, 2049)
	X, E = _operands(4, 1000, 64, ldx=68)
	with pytest.raises(ValueError, match=r"ldx = 68.*multiple of 8"):
		ops.score_topk_few(X, E, 1000, 10)
	with pytest.raises(ValueError, match=r"ldx = 68.*multiple of 8"):
		ops.score_rows_few(X, E, 1000)
	X, E = _operands(17, 1000, 2048)
	with pytest.raises(ValueError, match=r"131072 bytes, above the LDS stage of 65536"):
		ops.score_topk_few(X, E, 1000, 10)
	X, E = _operands(4, 1000, 64)
	with pytest.raises(ValueError, match="packed"):
		ops.score_topk_few(X, E[:992], 1000, 10)
	with pytest.raises(TypeError):
		ops.score_topk_few(X.float(), E, 1000, 10)
	with pytest.raises(_lib.AnncurHipError):                  # valid arguments on CPU tensors: there is no CPU path
		ops.score_topk_few(X, E, 1000, 10)
	with pytest.raises(_lib.AnncurHipError):
		ops.score_rows_few(X, E, 1000)


def test_few_ok_and_few_plan_at_their_boundaries():
	from anncur_amd import _lib, ops
	ok = ops.score_topk_few_ok
	assert ok(1, 100000, 256, 100) and ok(64, 100000, 512, 100) and not ok(65, 100000, 256, 100) and not ok(0, 100000, 256, 100)
	assert ok(16, 100000, 2048, 100) and not ok(17, 100000, 2048, 100) and not ok(16, 100000, 2176, 100)      # the LDS stage: 16 ceil(Q/16) Kp 2 <= 65536
	assert ok(32, 100000, 1024, 100) and not ok(33, 100000, 1024, 100) and ok(48, 100000, 640, 100) and not ok(49, 100000, 640, 100)
	assert not ok(4, 100000, 300, 100) and not ok(4, 100000, 576, 100)                                          # padded_k values only
	assert ok(4, 5000, 64, _lib.MAX_TOPK) and not ok(4, 5000, 64, _lib.MAX_TOPK + 1) and ok(4, 77, 64, 77) and not ok(4, 77, 64, 78) and not ok(4, 77, 64, 0)
	assert ok(1, (1 << 31) - 2, 64, 1) and not ok(1, (1 << 31) - 1, 64, 1)
	lib = _lib.load()
	assert lib.anncur_score_topk_few_workspace_bytes(65, 1000, 64, 10) == 0
	p = ops.few_plan(16, 100000, 256, 100)
	assert p["tiles"] == 6250 and p["groups"] == 1563 and p["query_subtiles"] == 1 and p["pitch"] == 100000 and p["cand_cap"] == 4352
	assert p["waves_per_workgroup"] == 4 and p["groups_per_wave"] == 1 and p["workgroups"] == 391 and (p["tiles_per_wave_min"], p["tiles_per_wave_max"]) == (2, 4)
	assert lib.anncur_score_topk_few_workspace_bytes(16, 100000, 256, 100) == p["scores_offset"] + 16 * p["pitch"] * 4
	assert p["gmax_offset"] == 1024 and p["scores_offset"] >= p["gmax_offset"] + 16 * 1563 * 4 and p["scores_offset"] % 256 == 0
	p = ops.few_plan(64, 1000003, 512, 2048)
	assert p["query_subtiles"] == 4 and p["cand_cap"] == 8192 and p["pitch"] == 1000032 and p["groups"] == 15626 and p["groups_per_wave"] == 8
	assert p["workgroups"] == 489 and p["tiles_per_wave_max"] == 32 and p["tiles_per_wave_min"] == p["tiles"] - 4 * 8 * (-(-15626 // 8) - 1)
	assert ops.few_plan(1, 1, 64, 1)["tiles"] == 1 and ops.few_plan(1, 17, 64, 1)["tiles_per_wave_min"] == 2
	with pytest.raises(ValueError, match="1..64"):
		ops.few_plan(65, 1000, 64, 10)
	with pytest.raises(ValueError, match="LDS stage"):
		ops.few_plan(64, 1000, 640, 10)


def test_score_kernels_use_no_scratch_and_keep_two_tiles_in_flight():
	"""From the built library's metadata (resource numbers only): the five bodies of few_score_kernel spill nothing, and at Kp = 256 a wave
	takes at most 256 of a SIMD's 512 registers per lane: two waves per SIMD, eight per CU, 64 KB of loads in flight."""
	sys.path.insert(0, os.path.join(ROOT, "scripts"))
	from check_kernel_resources import parse_kernel_notes
	from isa_tools import kernel_notes
	from anncur_amd import _lib
	kernels = [k for text in kernel_notes(_lib.LIB_PATH) for k in parse_kernel_notes(text) if "few_score_kernel" in k[".name"]]
	assert len(kernels) == 5, [k[".name"] for k in kernels]
	for k in kernels:
		assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
	k256 = [k for k in kernels if "ILi8ELb0EE" in k[".name"]]
	assert len(k256) == 1 and k256[0][".vgpr_count"] <= 256


def test_new_symbols_are_declared_and_exported():
	from anncur_amd import _lib
	lib = _lib.load()
	src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anncur_hip.h")).read(), flags=re.S)
	for name, n_args in NEW_SYMBOLS.items():
		assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
	assert "#define ANNCUR_FEW_MAX_Q 64" in src and "#define ANNCUR_FEW_STAGE_BYTES 65536" in src
