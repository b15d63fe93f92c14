"""Host side of the overlap counts (no GPU): the set reference on hand cases, what anncur_overlap_counts refuses before any
launch, the checks of ops.overlap_counts(mapped_host_out=) / ops.copy_to_mapped_host that need no device, and the pool's list and pairs.

A pinned tensor cannot be made without a device, so of the mapped_host_out / copy_to_mapped_host checks only "an unpinned tensor is refused,
before the operands are looked at" is here; the wrong dtype, shape and stride of a PINNED tensor and the size mismatch are in
tests/test_gpu_overlap_exact.py::test_mapped_host_arguments_are_validated."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from overlap_numpy import first_pos, overlap_ref  # noqa: E402


# ------------------------------------------------------------------ the reference
def test_reference_on_hand_cases():
	a, b = np.array([[5, 5, 7]]), np.array([[5, 9, 9]])
	assert overlap_ref(a, b, [(3, 3)]).tolist() == [[1]]                                   # a repeated id is one member of the set
	assert overlap_ref(a, b, [(0, 3), (3, 0), (0, 0), (1, 1), (2, 1), (3, 1)]).tolist() == [[0], [0], [0], [1], [1], [1]]
	assert overlap_ref(b, a, [(3, 3), (1, 3), (3, 2)]).tolist() == [[1], [1], [1]]
	pads = np.array([[-1, -1, -1], [3, -1, 4]])
	other = np.array([[-1, 3, -1], [-1, 4, 3]])
	assert overlap_ref(pads, other, [(3, 3), (3, 2), (1, 3)]).tolist() == [[0, 2], [0, 1], [0, 1]]      # a pad-only row; -1 in both lists adds nothing
	assert overlap_ref(np.array([[-2, -2 ** 31, 0]]), np.array([[-2 ** 31, -2, 0]]), [(3, 3), (2, 2)]).tolist() == [[1], [0]]
	big = 2 ** 31 - 1
	assert overlap_ref(np.array([[big, 0]], dtype=np.int32), np.array([[0, big]], dtype=np.int32), [(2, 2), (1, 1), (1, 2)]).tolist() == [[2], [0], [1]]
	out = overlap_ref(np.zeros((0, 4), dtype=np.int32), np.zeros((0, 2), dtype=np.int32), [(1, 1), (4, 2)])
	assert out.shape == (2, 0) and out.dtype == np.int32
	assert overlap_ref(a, b, []).shape == (0, 1)
	with pytest.raises(AssertionError):
		overlap_ref(a, b, [(4, 1)])


def test_first_pos():
	row = np.array([9, 4, -1, 4, 9, 0, -1], dtype=np.int32)
	assert [first_pos(row, x) for x in (9, 4, 0, 7, -1, -2)] == [0, 1, 5, 7, 7, 7]
	assert first_pos(row[:0], 3) == 0


def test_reference_counts_an_id_at_its_first_positions():
	"""The statement the kernels implement, against the set formula: an id counts for (ka, kb) iff ka is past its first position in a and
	kb past its first position in b."""
	rng = np.random.default_rng(11)
	for _ in range(200):
		la, lb = rng.integers(1, 12, 2)
		a, b = rng.integers(-2, 8, la), rng.integers(-2, 8, lb)
		ka, kb = rng.integers(0, la + 1), rng.integers(0, lb + 1)
		want = sum(1 for x in set(a.tolist()) if x >= 0 and first_pos(a, x) < ka and first_pos(b, x) < kb)
		assert overlap_ref(a[None], b[None], [(ka, kb)])[0, 0] == want


# ------------------------------------------------------------------ the C entry point: refusals before any launch
def test_c_entry_refuses_bad_arguments():
	from anncur_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(256)      # never dereferenced: every case below fails a host check
	i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

	def call(la=100, lb=200, Q=5, ka=(10,), kb=(20,), n_pairs=None, a=p, b=p, common=p, null_ka=False, null_kb=False):
		return lib.anncur_overlap_counts(a, la, b, lb, Q, None if null_ka else i32(*ka), None if null_kb else i32(*kb),
										 len(ka) if n_pairs is None else n_pairs, common, None)
	many = tuple([1] * 65)
	for kw, msg in ((dict(la=0, ka=(0,)), b"list lengths must be in 1..4096"), (dict(lb=0, kb=(0,)), b"list lengths must be in 1..4096"),
					(dict(la=4097), b"list lengths must be in 1..4096"), (dict(lb=4097), b"list lengths must be in 1..4096"),
					(dict(la=-1), b"list lengths must be in 1..4096"),
					(dict(n_pairs=0), b"n_pairs must be in 1..64"), (dict(ka=many, kb=many), b"n_pairs must be in 1..64"), (dict(n_pairs=-1), b"n_pairs must be in 1..64"),
					(dict(ka=(101,)), b"pair 0 prefix lengths (101,20) exceed list lengths (100,200)"),
					(dict(ka=(5, 100), kb=(200, 201)), b"pair 1 prefix lengths (100,201) exceed list lengths (100,200)"),
					(dict(ka=(-1,)), b"pair 0 prefix lengths (-1,20)"), (dict(ka=(3, 3, 3), kb=(0, 0, -5)), b"pair 2 prefix lengths (3,-5)"),
					(dict(la=128, lb=128, ka=(129,), kb=(1,)), b"pair 0 prefix lengths (129,1) exceed list lengths (128,128)"),
					(dict(Q=-1), b"bad Q"), (dict(Q=2 ** 31 - 1), b"bad Q"),
					(dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"), (dict(common=None), b"null pointer"),
					(dict(null_ka=True), b"null pointer"), (dict(null_kb=True), b"null pointer")):
		assert call(**kw) == -1 and msg in lib.anncur_last_error(), (kw, lib.anncur_last_error())
	# Q = 0: nothing to do, and an empty tensor's data pointer is null -- but the shapes and the pairs are still checked
	assert call(Q=0) == 0 and call(Q=0, a=None, b=None, common=None) == 0
	assert call(Q=0, ka=(101,)) == -1 and call(Q=0, lb=4097) == -1 and call(Q=0, null_ka=True) == -1
	# the limits themselves pass the host checks
	assert call(Q=0, la=4096, lb=4096, ka=(4096,) * 64, kb=(4096,) * 64) == 0 and call(Q=0, la=1, lb=1, ka=(0,), kb=(0,)) == 0


def test_copy_bytes_refusals_before_any_launch():
	from anncur_amd import _lib
	lib = _lib.load()
	p = ctypes.c_void_p(256)
	assert lib.anncur_copy_bytes(None, None, 0, None) == 0                                  # zero bytes: nothing to do, whatever the pointers
	for src, dst, msg in ((None, p, b"null pointer"), (p, None, b"null pointer"), (ctypes.c_void_p(264), p, b"16-byte aligned"),
						  (p, ctypes.c_void_p(257), b"16-byte aligned")):
		assert lib.anncur_copy_bytes(src, dst, 64, None) == -1 and msg in lib.anncur_last_error(), (src, dst, lib.anncur_last_error())


# ------------------------------------------------------------------ ops: what is checked before any device
def test_unpinned_host_tensors_are_refused_before_the_operands():
	from anncur_amd import _lib, ops
	a, b = torch.zeros((5, 10), dtype=torch.int32), torch.zeros((5, 20), dtype=torch.int32)
	out = torch.zeros((2, 5), dtype=torch.int32)            # right dtype, shape and stride, but pageable
	assert not out.is_pinned()
	with pytest.raises(ValueError, match="contiguous pinned int32 host tensor"):
		ops.overlap_counts(a, b, [(1, 1), (2, 2)], mapped_host_out=out)
	with pytest.raises(ValueError, match="contiguous pinned host tensor"):
		ops.copy_to_mapped_host(a, torch.zeros((5, 10), dtype=torch.int32))
	with pytest.raises(_lib.AnncurHipError, match="no CPU fallback"):      # valid arguments on CPU tensors: there is no CPU path
		ops.overlap_counts(a, b, [(1, 1)])


# ------------------------------------------------------------------ the pool's list and pairs
def test_pool_pairs_and_pool_list():
	from anncur_amd import retrieval as R
	assert R.pool_pairs([(1, 100), (10, 100), (10, 500)], 37) == [(1, 137), (10, 137), (10, 537)]
	assert R.pool_pairs([], 37) == [] and R.pool_pairs([(5, 7)], 0) == [(5, 7)]
	anc = np.array([7, 3, 2 ** 31 - 1], dtype=np.int64)
	retrieved = torch.tensor([[3, 9, 8, -1], [1, 0, 7, 5]], dtype=torch.int64)
	L = R.pool_list(anc, retrieved)
	assert L.dtype == torch.int32 and tuple(L.shape) == (2, 7) and L.is_contiguous() and L.device == retrieved.device
	assert L.tolist() == [[7, 3, 2 ** 31 - 1, 3, 9, 8, -1], [7, 3, 2 ** 31 - 1, 1, 0, 7, 5]]      # anchors first, in the order given; nothing deduplicated
	L0 = R.pool_list(np.zeros(0, dtype=np.int64), retrieved.to(torch.int32))
	assert L0.dtype == torch.int32 and L0.tolist() == retrieved.tolist()
	assert tuple(R.pool_list([4, 5], torch.zeros((0, 3), dtype=torch.int32)).shape) == (0, 5)
	# the prefix of length n_anc + k_retvr is the pool of a cell: the set formula over it, with the repeated anchor counted once
	exact = np.array([[3, 7, 9, 100], [5, 7, 2, 2 ** 31 - 1]])
	got = overlap_ref(exact, L.numpy(), R.pool_pairs([(2, 0), (3, 2), (4, 4)], 3))
	assert got.tolist() == [[2, 1], [3, 1], [3, 3]]
	# a pool is one list of the overlap kernel: never longer than it takes
	assert R.OVERLAP_MAX_LIST == 4096 and R.pool_cell_limit(10 ** 6) <= 4096 and R.pool_cell_limit(50) == 50
	lim = R.pool_cell_limit(10 ** 6)
	assert R.split_pool_cells([(1, 100), (1, lim - 37), (1, lim - 36)], 37, 10 ** 6) == ([(1, 100), (1, lim - 37)], [(1, lim - 36)])
