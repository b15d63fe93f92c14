"""Host side of the adaptive multi-round search: the limits of AdaptiveSearcher.search, of ops.lstsq_rows and of
ops.sort_id_rows, each a ValueError that names the limit and is raised before the scorer or the GPU is touched; the workspace size and
the limits of the C entry points, which answer without a device.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch


def _index(m=5000, kq=16, anchors=(2, 5, 700, 4999)):
	from anncur_amd.cur import CURRowIndex
	index = CURRowIndex.__new__(CURRowIndex)     # (the limits need the item count, the anchor-query count and the anchor ids only)
	index.R, index.m, index.col_idxs = torch.zeros(kq, m), m, list(anchors)
	return index


def test_adaptive_limits_are_host_checks_before_the_first_scorer_call():
	from anncur_amd import _lib
	from anncur_amd.search import AdaptiveResult, AdaptiveSearcher
	assert (_lib.MAX_TOPK, _lib.LSTSQ_MAX_G, _lib.LSTSQ_MAX_KQ) == (2048, 512, 4096)
	calls = []
	scorer = lambda q, i: calls.append(1)
	s = AdaptiveSearcher(_index(), scorer)
	assert s.kc == 4 and s.kq == 16 and s.ridge == 0.0 and s._excl.e_max == 4 and s._shared.ids.tolist() == [2, 5, 700, 4999]
	q = np.arange(3)
	for k_step, n_rounds in ((10, 0), (0, 2), (10, -1)):
		with pytest.raises(ValueError, match=rf"n_rounds >= 1 and k_step >= 1 \(got n_rounds = {n_rounds}, k_step = {k_step}\)"):
			s.search(q, 5, k_step, n_rounds)
	with pytest.raises(ValueError, match=r"kc \+ n_rounds \* k_step = 4 \+ 4 \* 512 = 2052 scored items per query.*min\(items, ANNCUR_MAX_TOPK\) = min\(5000, 2048\) = 2048"):
		s.search(q, 5, 512, 4)
	with pytest.raises(ValueError, match=r"4 \+ 2 \* 50 = 104.*min\(100, 2048\) = 100"):
		AdaptiveSearcher(_index(m=100, anchors=(2, 5, 70, 99)), scorer).search(q, 5, 50, 2)
	with pytest.raises(ValueError, match=r"1 <= k <= min\(pool size, ANNCUR_MAX_TOPK\) = min\(44, 2048\) = 44 \(got k = 45\)"):
		s.search(q, 45, 10, 4)
	with pytest.raises(ValueError, match=r"got k = 0"):
		s.search(q, 0, 10, 4)
	# g = min(kc + (n_rounds - 1) k_step, kq): 4 + 600 = 604 against kq = 1000
	wide = AdaptiveSearcher(_index(kq=1000), scorer)
	with pytest.raises(ValueError, match=r"min\(kc \+ \(n_rounds - 1\) \* k_step, kq\) = min\(604, 1000\) = 604, above ANNCUR_LSTSQ_MAX_G = 512"):
		wide.search(q, 5, 600, 2)
	with pytest.raises(ValueError, match=r"kq = 5000 anchor queries, above ANNCUR_LSTSQ_MAX_KQ = 4096"):
		AdaptiveSearcher(_index(kq=5000), scorer).search(q, 5, 100, 2)
	assert calls == []
	# ... and none of them applies to a single round or to kq <= 512: the call then reaches the scorer
	for searcher, args in ((wide, (5, 600, 1)), (s, (5, 600, 3))):
		with pytest.raises(Exception) as e:
			searcher.search(q, *args)
		assert not isinstance(e.value, ValueError)
	assert len(calls) == 2
	with pytest.raises(ValueError, match="ridge = -1.0, need ridge >= 0"):
		AdaptiveSearcher(_index(), scorer, ridge=-1.0)
	with pytest.raises(ValueError, match="strictly ascending"):
		AdaptiveSearcher(_index(anchors=(5, 2)), scorer)
	assert AdaptiveResult._fields == ("values", "indices", "n_scored", "n_fallback", "trace")


def test_lstsq_rows_limits_name_the_constant():
	from anncur_amd import _lib, ops
	for (n, kq), msg in (((2049, 16), r"2049 scored items per query, outside 1\.\.ANNCUR_MAX_TOPK = 2048"),
						 ((0, 16), r"0 scored items per query"),
						 ((10, 4097), r"kq = 4097 anchor queries, outside 1\.\.ANNCUR_LSTSQ_MAX_KQ = 4096"),
						 ((513, 600), r"g = min\(n, kq\) = min\(513, 600\) = 513, above ANNCUR_LSTSQ_MAX_G = 512")):
		with pytest.raises(ValueError, match=msg):
			ops._lstsq_check(3, n, kq, 0.0)
	for ridge in (-0.5, float("nan")):
		with pytest.raises(ValueError, match="need ridge >= 0"):
			ops._lstsq_check(3, 10, 16, ridge)
	assert ops._lstsq_check(3, 2048, 512, 0.0) is None and ops._lstsq_check(3, 512, 4096, 1.0) is None
	with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):     # there is no CPU path
		ops.lstsq_rows(torch.zeros(10, 4), torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, 3))
	with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):
		ops.sort_id_rows(torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, 3))
	with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):
		ops.exclusion_from_sorted_rows(torch.zeros((2, 3), dtype=torch.int32))


def test_c_entry_points_answer_size_and_limits_without_a_device():
	from anncur_amd import _lib
	lib = _lib.load()
	ws = lib.anncur_lstsq_rows_workspace_bytes
	assert ws(1, 16, 16) == 17 * 16 * 8 and ws(7, 17, 100) == 7 * 33 * 32 * 8 and ws(3, 300, 100) == 3 * 113 * 112 * 8     # (gp + 1) gp doubles, gp = ceil16(min(n, kq))
	assert ws(10, 512, 1536) == 10 * 513 * 512 * 8 and ws(10 ** 4, 512, 500) == 10 ** 4 * 513 * 512 * 8                   # (size_t: beyond 2^32)
	assert ws(1, 513, 513) == 0 and ws(1, 2049, 16) == 0 and ws(1, 16, 4097) == 0 and ws(1, 0, 16) == 0 and ws(-1, 16, 16) == 0
	assert ws(1, 2048, 512) > 0 and ws(1, 512, 4096) > 0 and ws(0, 16, 16) == 0
	null = ctypes.c_void_p(None)
	bad = [(600, 513, 0.0, "min\\(n, kq\\) <= 512"), (16, 16, -1.0, "ridge >= 0")]
	for kq, n, ridge, msg in bad:
		assert lib.anncur_lstsq_rows(null, kq, 10, kq, null, n, null, n, 1, n, ridge, null, kq, null, null, 0, null) == -1     # ANNCUR_E_INVALID before any pointer is read
		import re
		assert re.search(msg, lib.anncur_last_error().decode())
	assert lib.anncur_lstsq_rows(null, 16, 10, 16, null, 16, null, 16, 0, 16, 0.0, null, 16, null, null, 0, null) == 0           # Q = 0: nothing to do
	assert lib.anncur_sort_id_rows(null, null, 4, 1, 2049, null, null, 4, null, null) == -1 and b"w <= 2048" in lib.anncur_last_error()
	assert lib.anncur_sort_id_rows(null, null, 4, 0, 4, null, null, 4, null, null) == 0
