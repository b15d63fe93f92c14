"""Host side of filtered retrieval (the `exclude=` argument of the top-k calls): no GPU needed."""
import numpy as np
import pytest
import torch

CPU = torch.device("cpu")


def _segments(ex, Q):
	"""The exclusion as a list of Q python lists."""
	ids = ex.ids.tolist()
	if ex.off is None:
		return [ids] * Q
	off = ex.off.tolist()
	assert len(off) == Q + 1 and off[0] == 0 and off[-1] == len(ids)
	return [ids[off[q]:off[q + 1]] for q in range(Q)]


def _check_types(ex):
	assert ex.ids.dtype == torch.int32 and ex.ids.dim() == 1 and ex.ids.is_contiguous()
	assert ex.off is None or (ex.off.dtype == torch.int64 and ex.off.is_contiguous())
	assert isinstance(ex.e_max, int)


@pytest.mark.parametrize("make", [list, tuple, np.asarray, torch.as_tensor, lambda x: np.asarray(x, dtype=np.int32)], ids=["list", "tuple", "numpy", "tensor", "int32"])
def test_exclusion_shared_list_is_sorted_and_deduplicated(make):
	from anncur_amd import ops
	ex = ops.exclusion(make([7, 3, 3, 99, 0, 7]), 4, 100, CPU)
	_check_types(ex)
	assert ex.off is None and ex.ids.tolist() == [0, 3, 7, 99] and ex.e_max == 4
	assert _segments(ex, 4) == [[0, 3, 7, 99]] * 4


def test_exclusion_per_query_lists():
	from anncur_amd import ops
	lists = [[5, 1, 5], [], np.array([9, 8, 7]), torch.tensor([2]), (4, 4, 4, 4), range(3)]
	ex = ops.exclusion(lists, 6, 10, CPU)
	_check_types(ex)
	assert ex.off.tolist() == [0, 2, 2, 5, 6, 7, 10]
	assert _segments(ex, 6) == [[1, 5], [], [7, 8, 9], [2], [4], [0, 1, 2]]
	assert ex.e_max == 3                      # the longest list AFTER de-duplication
	# -1 is not padding in the ragged form
	with pytest.raises(ValueError, match="negative id -1"):
		ops.exclusion([[1, -1], [2]], 2, 10, CPU)


def test_exclusion_padded_2d_array():
	from anncur_amd import ops
	a = np.array([[3, -1, 1, 3], [-1, -1, -1, -1], [0, 1, 2, 9]])
	for form in (a, a.astype(np.int32), torch.from_numpy(a)):
		ex = ops.exclusion(form, 3, 10, CPU)
		_check_types(ex)
		assert _segments(ex, 3) == [[1, 3], [], [0, 1, 2, 9]] and ex.e_max == 4
	assert ops.exclusion(np.zeros((3, 0), dtype=np.int64), 3, 10, CPU).e_max == 0
	with pytest.raises(ValueError, match="negative id -2"):
		ops.exclusion(np.array([[1, -2]]), 1, 10, CPU)


def test_exclusion_empty_forms_and_pass_through():
	from anncur_amd import ops
	assert ops.exclusion(None, 3, 10, CPU).e_max == 0
	ex = ops.exclusion([], 3, 10, CPU)
	assert ex.off is None and ex.ids.numel() == 0 and ex.e_max == 0
	ex = ops.exclusion([[]] * 3, 3, 10, CPU)
	assert ex.off.tolist() == [0, 0, 0, 0] and ex.ids.numel() == 0 and ex.e_max == 0
	# an already normalised exclusion passes through untouched: an index can cache it
	ex = ops.exclusion([[1], [2, 3]], 2, 10, CPU)
	assert ops.exclusion(ex, 2, 10, CPU) is ex
	with pytest.raises(ValueError, match="built for 2 queries"):
		ops.exclusion(ex, 3, 10, CPU)
	shared = ops.exclusion([4, 2], 2, 10, CPU)
	assert ops.exclusion(shared, 77, 10, CPU) is shared          # a shared list fits any number of queries
	assert isinstance(ex, tuple) and len(ex) == 3 and ex[2] == ex.e_max == 2


def test_exclusion_every_value_error():
	from anncur_amd import ops
	with pytest.raises(ValueError, match="holds the id 10, but there are only 10 items"):
		ops.exclusion([0, 10], 2, 10, CPU)
	with pytest.raises(ValueError, match="list 1 holds the id 12"):
		ops.exclusion([[0], [12]], 2, 10, CPU)
	with pytest.raises(ValueError, match="row 0 holds the id 10"):
		ops.exclusion(np.array([[10, -1]]), 1, 10, CPU)
	assert ops.exclusion([0, 10], 2, None, CPU).ids.tolist() == [0, 10]   # no item count: no upper check (ops.filter_topk)
	with pytest.raises(ValueError, match="negative id -1"):
		ops.exclusion([3, -1], 2, 10, CPU)                                 # -1 pads only the 2-D form
	with pytest.raises(ValueError, match="negative id -5"):
		ops.exclusion([[3], [-5]], 2, 10, CPU)
	with pytest.raises(ValueError, match="3 per-query lists, the call has 2 queries"):
		ops.exclusion([[1], [2], [3]], 2, 10, CPU)
	with pytest.raises(ValueError, match="2 rows, the call has 3 queries"):
		ops.exclusion(np.array([[1, 2], [3, 4]]), 3, 10, CPU)
	with pytest.raises(ValueError, match="1-D .* or 2-D"):
		ops.exclusion(np.zeros((2, 2, 2), dtype=np.int64), 2, 10, CPU)
	with pytest.raises(ValueError, match="integer item ids"):
		ops.exclusion([1.5, 2.0], 2, 10, CPU)
	with pytest.raises(ValueError, match="flat list"):
		ops.exclusion([[1], [[2]]], 2, 10, CPU)


def test_kc_arithmetic_and_over_limit_error():
	from anncur_amd import _lib, ops
	assert ops.filtered_k(100, 0, 100000) == 100 and ops.filtered_k(100, 128, 100000) == 228
	assert ops.filtered_k(10, 5, 15) == 15 and ops.filtered_k(2000, 48, 100000) == _lib.MAX_TOPK
	with pytest.raises(ValueError) as e:
		ops.filtered_k(10, 6, 15)
	assert "10 + 6 = 16" in str(e.value) and "min(15, 2048) = 15" in str(e.value) and "rebuild the index without those items" in str(e.value)
	with pytest.raises(ValueError, match=r"min\(100000, 2048\) = 2048.*rebuild the index"):
		ops.filtered_k(2000, 49, 100000)
	# the bf16x3 sweep: the exclusion widens the retrieval, the rescore margin stays that of k
	assert ops.split_candidates(100000, 100, n_excl=128) == 100 + 128 + ops.split_rescore_extra(100)
	assert ops.split_candidates(100000, 100, extra=0, n_excl=7) == 107
	assert ops.split_candidates(100000, 2000, n_excl=40) == _lib.MAX_TOPK and ops.split_candidates(50, 10, n_excl=30) == 50


def test_exclude_none_leaves_the_route_arguments_as_today(monkeypatch):
	from anncur_amd import cur, ops
	seen = []
	monkeypatch.setattr(ops, "fused_supported", lambda Q, I, Kp, k: seen.append((Q, I, Kp, k)) or True)
	# nothing to exclude -> no Exclusion, kc == k: the calls take today's path (no filter launch)
	for nothing in (None, [], [[]] * 7, np.full((7, 3), -1), ops.exclusion([[]] * 7, 7, 5000, CPU)):
		assert cur._exclusion_arg(nothing, 7, 5000, 100, CPU) == (None, 100)
	res = ops.TopK("v", "i")
	assert cur._filtered(res, None, 100) is res
	assert ops.split_candidates(100000, 100) == 116 and ops.split_candidates(100000, 100, None) == 116
	sp = cur._SplitOperands(512, None, None)
	assert sp.takes(7, 100000, 100) and sp.takes(7, 100000, 100, None)
	assert seen == [(7, 100000, 512, 116)] * 2
	# with an exclusion: k + e_max through the bf16 route, k + e_max + the margin of k through the bf16x3 sweep
	excl, kc = cur._exclusion_arg([[1, 2, 3]] + [[]] * 6, 7, 100000, 100, CPU)
	assert excl.e_max == 3 and kc == 103
	del seen[:]
	assert sp.takes(7, 100000, 100, excl) and seen == [(7, 100000, 512, 119)]
	assert not sp.takes(7, 100000, 2046, excl)                  # k + e_max above MAX_TOPK
	with pytest.raises(ValueError, match="rebuild the index"):
		cur._exclusion_arg(list(range(60)), 7, 150, 100, CPU)


def test_filter_topk_refuses_cpu_tensors_and_signature_is_bound():
	from anncur_amd import _lib, ops
	assert "anncur_filter_topk" in _lib.SIGNATURES and len(_lib.SIGNATURES["anncur_filter_topk"][1]) == 12
	assert hasattr(_lib.load(), "anncur_filter_topk")
	with pytest.raises(_lib.AnncurHipError):
		ops.filter_topk(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), [1], 2)
