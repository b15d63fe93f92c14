"""ops.select_pivoted / anncur_select_pivoted on the device.

Exact integer data: kq = 64 and item i = s_i H[:, i mod 64], H the 64 x 64 Hadamard matrix, s_i small integers (tests/pivot_numpy.py); where k = 80
exceeds the rank, 32 zero rows are appended (kq = 96), because the call's own limit is k <= kq.  Every
q_t is +-1/8, every c_i an exact multiple of 8 s_i, exactly 0 for an item orthogonal to q_t in ANY summation order, and an item parallel to
q_t drops to d_i = 0 exactly, so ids, gain = 64 s^2 and n_sel are known in closed form and asserted for equality -- at every edge of the step
kernel's slices, with poisoned pads, outputs and workspace, unaligned rows, bf16, and columns of NaN / inf.
Generic data (the three shapes of tests/test_cpu_pivot_host.py, fp32 and bf16): the numpy restatement's minimum gap is asserted >= 2^-30
first -- a condition on the reference alone --, then ids for equality and |gain_dev - gain_ref| <= 2^-40 d_first: the two differ by the
order of their sums only, (kq + 4 t) 2^-53 <= 2^-44 at these sizes, a 16-fold margin.  Needs an MI355X."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pivot_numpy as pn  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _scales(m, seed=5):
	rng = np.random.default_rng(seed)
	s = rng.integers(1, 10, m)                                  # 9 values on 64 directions: several directions tie exactly, some do not
	s[rng.choice(m, m // 8, replace=False)] *= -1
	return s


def _run(ops, R, k):
	ids, gains, n_sel = ops.select_pivoted(R, k)
	return ids.cpu().numpy().astype(np.int64), gains.cpu().numpy(), n_sel


def _check_closed_form(ops, scales, k, dtype=torch.float32, never=(), R=None):
	"""kq = 64 while k <= 64; a k above the rank gets kq = 96 (32 zero rows), so that it stays inside the call's limit k <= kq."""
	want_ids, want_gains, want_n = pn.hadamard_closed_form(scales, k, never=never)
	if R is None:
		R = torch.from_numpy(pn.hadamard_items(scales, 64 if k <= 64 else 96).astype(np.float32)).cuda().to(dtype)
	ids, gains, n_sel = _run(ops, R, k)
	assert n_sel == want_n
	assert np.array_equal(ids, want_ids), (ids, want_ids)
	assert np.array_equal(gains, want_gains)
	return ids, gains, n_sel


def test_rank_64_of_323_items_with_ties_and_the_tail(ops):
	scales = _scales(323)
	ids, gains, n_sel = _check_closed_form(ops, scales, 80)
	assert n_sel == 64 and (ids[64:] == -1).all() and (gains[64:] == 0.0).all()
	assert 1 < len(set(gains[:64].tolist())) < 64                  # exact ties between directions, and not only ties
	_check_closed_form(ops, scales, 1)
	_check_closed_form(ops, scales, 64)


@pytest.mark.parametrize("where", ["first", "last"])
def test_first_winner_at_either_end(ops, where):
	scales = _scales(323)
	p = 0 if where == "first" else 322
	scales[p] = 50
	ids, _, _ = _check_closed_form(ops, scales, 80)
	assert ids[0] == p


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_winner_in_every_slice_and_in_the_ragged_tail(ops, dtype):
	"""m from the step kernel's own slice: three full slices and a tail of 5 items (no multiple of the 4- or 8-item vector); the first four
	winners sit one per slice -- mid-slice, just past a slice's start, a slice's last item, the tail's last item."""
	S = ops.select_pivoted_slice_items(DTYPES[dtype])
	assert S > 0 and S % 64 == 0
	m = 3 * S + 5
	scales = _scales(m)
	at = [7, S + S // 2 + 1, 3 * S - 1, m - 1]
	assert len({i % 64 for i in at}) == 4 and [i // S for i in at] == [0, 1, 2, 3]
	for rank, i in enumerate(at):
		scales[i] = 40 - rank
	ids, _, n_sel = _check_closed_form(ops, scales, 64, DTYPES[dtype])
	assert list(ids[:4]) == at and n_sel == 64


def _raw(lib, R_ptr, dtype_code, ldr, kq, m, k, ids, gains, n_sel, ws, ws_bytes=None):
	return lib.anncur_select_pivoted(ctypes.c_void_p(R_ptr), dtype_code, ldr, kq, m, k, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(gains.data_ptr()),
									 ctypes.c_void_p(n_sel.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes,
									 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _poisoned(k, nbytes):
	"""Outputs and a private 256-byte aligned workspace, every byte 0xff."""
	ids = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")                      # 0xffffffff
	gains = torch.full((k + 2,), -1, dtype=torch.int64, device="cuda").view(torch.float64)  # 0xff..ff: a NaN
	n_sel = torch.full((3,), -1, dtype=torch.int32, device="cuda")
	buf = torch.full((nbytes + 256,), 0xff, dtype=torch.uint8, device="cuda")
	off = (-buf.data_ptr()) % 256
	return ids, gains, n_sel, buf[off:off + nbytes]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pitch_pad_of_nan_and_poisoned_outputs_and_workspace(ops, dtype):
	"""ldr > m with NaN in the pad, 0xff in every output and workspace byte: the answer is the closed form, and nothing is written past
	position k of the outputs."""
	from anncur_amd import _lib
	lib = _lib.load()
	m, ldr, k = 323, 336, 80
	scales = _scales(m)
	want_ids, want_gains, want_n = pn.hadamard_closed_form(scales, k)
	Rp = torch.full((96, ldr), float("nan"), dtype=torch.float32, device="cuda")
	Rp[:, :m] = torch.from_numpy(pn.hadamard_items(scales, 96).astype(np.float32)).cuda()
	Rp = Rp.to(DTYPES[dtype])
	ids, gains, n_sel, ws = _poisoned(k, lib.anncur_select_pivoted_workspace_bytes(m, 96, k))
	assert _raw(lib, Rp.data_ptr(), ops._DT[DTYPES[dtype]], ldr, 96, m, k, ids, gains, n_sel, ws) == 0
	torch.cuda.synchronize()
	assert n_sel.tolist() == [want_n, -1, -1]
	assert np.array_equal(ids.cpu().numpy()[:k], want_ids) and ids[k:].tolist() == [-1, -1]
	assert np.array_equal(gains.cpu().numpy()[:k], want_gains) and gains[k:].view(torch.int64).tolist() == [-1, -1]
	# the same through ops on the padded view (rows keep their pitch)
	got = _run(ops, Rp[:, :m], k)
	assert got[2] == want_n and np.array_equal(got[0], want_ids) and np.array_equal(got[1], want_gains)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rows_that_are_not_16_byte_aligned(ops, dtype):
	"""R starts one element into its allocation and has an odd pitch: no row is 16-byte aligned, and their misalignments differ."""
	S = ops.select_pivoted_slice_items(DTYPES[dtype])
	m = S + 37
	ldr = m + 2 + (m % 2 == 0)                                   # odd
	scales = _scales(m)
	scales[m - 1] = 30
	flat = torch.full((64 * ldr + 1,), float("nan"), dtype=torch.float32, device="cuda").to(DTYPES[dtype])
	R = flat[1:].view(64, ldr)[:, :m]
	R.copy_(torch.from_numpy(pn.hadamard_items(scales).astype(np.float32)).cuda().to(DTYPES[dtype]))
	assert R.data_ptr() % 16 != 0 and (ldr * R.element_size()) % 16 != 0 and R.stride(0) == ldr
	ids, _, _ = _check_closed_form(ops, scales, 64, DTYPES[dtype], R=R)
	assert ids[0] == m - 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_nan_and_inf_columns_are_never_selected(ops, dtype):
	"""Column 3 all NaN, column 70 holding one +inf, and column 130 = -inf throughout: none is taken; the rest of the answer is that of the
	data without them.  Item 3 would have been the first pick."""
	scales = _scales(323)
	scales[3] = 60
	R = torch.from_numpy(pn.hadamard_items(scales, 96).astype(np.float32)).cuda()
	R[:, 3] = float("nan")
	R[5, 70] = float("inf")
	R[:, 130] = float("-inf")
	ids, _, n_sel = _check_closed_form(ops, scales, 80, DTYPES[dtype], never=(3, 70, 130), R=R.to(DTYPES[dtype]))
	assert n_sel == 64 and not np.isin([3, 70, 130], ids).any()


def test_rank_below_k_stops_at_the_rank(ops):
	"""Directions 40.. hold zeros only: n_sel = 40, reached through d_p = 0 exactly."""
	scales = _scales(323)
	scales[np.arange(323) % 64 >= 40] = 0
	_, _, n_sel = _check_closed_form(ops, scales, 64)
	assert n_sel == 40
	_, _, n_sel = _check_closed_form(ops, np.zeros(100, dtype=np.int64), 5)       # R = 0: nothing to take
	assert n_sel == 0


# ------------------------------------------------------------------ generic data against the restatement
@functools.lru_cache(maxsize=None)
def _generic(case, dtype):
	kq, m, k, rank, noise, seed = pn.GENERIC[case]
	R = torch.from_numpy(pn.low_rank(kq, m, rank, noise, seed))
	if dtype == "bf16":
		R = R.bfloat16()
	ref = pn.select(R.float().numpy(), k)                        # the reference sees the values the device sees
	return R.cuda(), k, ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(pn.GENERIC)))
def test_generic_data_equals_the_restatement(ops, case, dtype):
	R, k, (want_ids, want_gains, want_n, gaps) = _generic(case, dtype)
	print(f"{tuple(R.shape)} {dtype}, k = {k}: minimum gap of the restatement {gaps.min():.3g}")
	assert want_n == k and gaps.min() >= 2.0 ** -30               # a condition on the reference alone
	ids, gains, n_sel = _run(ops, R, k)
	assert n_sel == k and np.array_equal(ids, want_ids)
	bound = 2.0 ** -40 * want_gains[0]
	err = np.abs(gains - want_gains).max()
	print(f"  max |gain_dev - gain_ref| = {err:.3g}, bound {bound:.3g}")
	assert err <= bound
	assert (np.diff(gains) <= bound).all()                        # non-increasing up to the same bound


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_reproducible_and_nested(ops, dtype):
	R, k, _ = _generic(0, dtype)
	a = ops.select_pivoted(R, k)
	b = ops.select_pivoted(R, k)
	assert a[2] == b[2] == k and torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
	for k2 in (1, 7, k - 1):
		c = ops.select_pivoted(R, k2)
		assert c[2] == k2 and torch.equal(c[0], a[0][:k2]) and torch.equal(c[1].view(torch.int64), a[1][:k2].view(torch.int64))


@pytest.mark.parametrize("case", range(len(pn.GENERIC)))
def test_the_selected_set_passes_the_item_side_solve(ops, case):
	"""Pivot-rule coherence: the stop rule is lstsq_rows' pivot rule, so the selected ids as one query's list give status 0."""
	R, k, _ = _generic(case, "fp32")
	ids, _, n_sel = ops.select_pivoted(R, k)
	assert n_sel == k
	Rt = R.t().contiguous()
	C = torch.from_numpy(np.random.default_rng(case).standard_normal((1, k)).astype(np.float32)).cuda()
	W, status = ops.lstsq_rows(Rt, ids[None, :].contiguous(), C)
	assert status.tolist() == [0] and torch.isfinite(W).all()


def test_limit_violations_leave_poisoned_outputs_untouched(ops):
	from anncur_amd import _lib
	lib = _lib.load()
	kq, m, k = 16, 100, 8
	R = torch.randn(kq, m, device="cuda")
	ids, gains, n_sel, ws = _poisoned(k, lib.anncur_select_pivoted_workspace_bytes(m, kq, k))

	def untouched():
		torch.cuda.synchronize()
		return (ids == -1).all().item() and (gains.view(torch.int64) == -1).all().item() and (n_sel == -1).all().item() and (ws == 0xff).all().item()
	call = lambda dtype=0, ldr=m, kq=kq, m=m, k=k, ws_bytes=None, ws=ws: _raw(lib, R.data_ptr(), dtype, ldr, kq, m, k, ids, gains, n_sel, ws, ws_bytes)
	for kw in (dict(k=0), dict(k=-1), dict(k=kq + 1), dict(m=4, k=5), dict(k=_lib.MAX_TOPK + 1, kq=4096, m=5000, ldr=5000), dict(kq=0), dict(kq=_lib.LSTSQ_MAX_KQ + 1),
			   dict(m=2 ** 31, ldr=2 ** 31), dict(m=0, ldr=0), dict(ldr=m - 1), dict(dtype=2)):
		assert call(**kw) == -1, kw
		assert untouched(), kw
	for kw in (dict(ws_bytes=ws.numel() - 1), dict(ws=ws[8:])):
		assert call(**kw) == -2, kw
		assert untouched(), kw
	assert call() == 0                                            # and the valid call on the same buffers goes through
	torch.cuda.synchronize()
	assert n_sel[0].item() == k and (ids[:k] >= 0).all().item() and ids[k:].tolist() == [-1, -1]
