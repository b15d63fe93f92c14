"""Host side of the shared-prefix seed of the incremental solve: the limits of anncur_lstsq_seed_shared, which answers without a
device, the checks of ops.LstsqState.seed_shared, each a ValueError that names the limit and is raised before any launch, the searcher's
switch, and the state size, which the seed leaves as it was.  No GPU needed."""
import ctypes
import re

import numpy as np
import pytest
import torch


def _state(kq=100, Q=3, cap=48, m=10, **kw):
	from anncur_amd import ops
	return ops.LstsqState(torch.zeros(m, kq), Q, cap, **kw)


def test_c_entry_point_answers_limits_without_a_device():
	from anncur_amd import _lib
	lib = _lib.load()
	null = ctypes.c_void_p(None)

	def seed(kq, n_sh, cap, ridge=0.0, Q=1, m=10, ldr=None):
		return lib.anncur_lstsq_seed_shared(null, kq if ldr is None else ldr, m, kq, null, n_sh, Q, cap, ridge, null, 0, null)
	for args, msg in (((64, 0, 32), r"1 <= n_sh <= min\(cap, kq\)"), ((64, 33, 32), r"1 <= n_sh <= min\(cap, kq\)"), ((16, 17, 32), r"1 <= n_sh <= min\(cap, kq\)"),
					  ((64, 8, 0), r"1 <= cap <= 512"), ((64, 8, 513), r"1 <= cap <= 512"), ((4097, 8, 16), r"1 <= kq <= 4096")):
		assert seed(*args) == -1 and re.search(msg, lib.anncur_last_error().decode()), args      # ANNCUR_E_INVALID before any pointer is read
	assert seed(64, 8, 32, ridge=-1.0) == -1 and b"ridge >= 0" in lib.anncur_last_error()
	assert seed(64, 8, 32, ridge=float("nan")) == -1 and b"ridge >= 0" in lib.anncur_last_error()
	assert seed(64, 8, 32, m=0) == -1 and b"m >= 1" in lib.anncur_last_error()
	assert seed(64, 8, 32, ldr=63) == -1 and b"ldr >= kq" in lib.anncur_last_error()
	assert seed(64, 8, 32, Q=-1) == -1 and b"Q >= 0" in lib.anncur_last_error()
	assert seed(64, 8, 32, Q=0) == 0                                                            # Q = 0: nothing to do
	assert seed(64, 32, 32, Q=0) == 0 and seed(32, 32, 64, Q=0) == 0                            # n_sh = cap and n_sh = kq are inside


def test_seed_shared_limits_are_raised_before_any_launch():
	from anncur_amd import _lib
	s = _state(kq=40, Q=3, cap=48, m=10)
	s.n = 16       # as after a call that absorbed 16 positions
	with pytest.raises(ValueError, match=r"16 positions are absorbed already: a state is seeded before its first extend \(\.n == 0\)"):
		s.seed_shared([1, 2, 3])
	s.n = 0
	with pytest.raises(ValueError, match=r"n_sh = 0 shared ids, outside 1\.\.min\(cap, kq\) = min\(48, 40\) = 40"):
		s.seed_shared([])
	with pytest.raises(ValueError, match=r"n_sh = 41 shared ids, outside 1\.\.min\(cap, kq\) = min\(48, 40\) = 40"):       # above kq
		s.seed_shared(np.arange(41) % 10)
	with pytest.raises(ValueError, match=r"n_sh = 17 shared ids, outside 1\.\.min\(cap, kq\) = min\(16, 100\) = 16"):      # above cap
		_state(kq=100, cap=16).seed_shared(torch.arange(17, dtype=torch.int32) % 10)
	for bad in (-1, 10):
		with pytest.raises(ValueError, match=rf"id {bad} outside \[0, m\) = \[0, 10\)"):
			s.seed_shared([0, 1, bad, 3])
	with pytest.raises(ValueError, match="flat list of integer item ids"):
		s.seed_shared([[0, 1], [2, 3]])
	with pytest.raises(ValueError, match="flat list of integer item ids"):
		s.seed_shared([0.5, 1.0])
	assert s.n == 0 and s._buf is None
	for ids in ([0, 1, 9, 3], np.array([0, 1, 1, 3]), torch.tensor([5, 4], dtype=torch.int32)):     # (duplicates are not a host error)
		with pytest.raises(_lib.AnncurHipError, match="need tensors on the GPU"):                    # every host check passed: there is no CPU path
			s.seed_shared(ids)
		assert s.n == 0 and s._buf is None


def test_searcher_stores_the_switch_and_it_defaults_to_true():
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher
	index = CURRowIndex.__new__(CURRowIndex)
	index.R, index.m, index.col_idxs = torch.zeros(16, 5000), 5000, [2, 5, 700, 4999]
	scorer = lambda q, i: None
	assert AdaptiveSearcher(index, scorer).seed_shared is True
	assert AdaptiveSearcher(index, scorer, incremental=True).seed_shared is True
	s = AdaptiveSearcher(index, scorer, incremental=True, seed_shared=False)
	assert s.seed_shared is False and s.incremental is True
	assert AdaptiveSearcher(index, scorer, incremental=True, seed_shared=True).seed_shared is True


def test_state_bytes_are_what_they_were():
	from anncur_amd import _lib
	sb = _lib.load().anncur_lstsq_state_bytes
	for cap in (1, 16, 17, 456, 512):
		capp = -(-cap // 16) * 16
		for Q in (1, 7, 10 ** 4):
			assert sb(Q, cap) == ((capp + 2) * capp + 16) * 8 * Q, (Q, cap)
