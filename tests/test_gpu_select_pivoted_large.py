"""ops.select_pivoted / anncur_select_pivoted at the callers' sizes: kq from 256 to the limit 4096 and m beyond the step kernel's
grid cap.  tests/test_gpu_select_pivoted.py stops at kq = 96 and m = 3 slices + 5; the loops and branches that only larger sizes enter are
entered here, with the same kind of assertion: equality of ids, gains and n_sel on exact data, outputs and workspace poisoned with 0xff.

Exact data: item i = s_i H_n[:, i mod n] in the first n of kq rows (tests/pivot_numpy.py), n a power of 4, so that q_t = +-1/sqrt(n) is a power
of two and every c_i, d_i is exact in any summation order; gain = n s^2.
  * every shape of the pick kernel's update: G = 4, 3 (uneven shares), 2, and G = 1 with one and with two passes of its loops over kq; a row
    tail of 3 in the step kernel's walk (kq = 603, 1027); kq = 4096, the limit.  What this data can NOT do: every Gram-Schmidt coefficient is
    an exact 0 on it, so the update subtracts nothing and a wrong update passes (the first mutation below).  It holds the pick, the column
    load, the norm, q_t's store and the step kernel's walk; the update is held by the generic data, which has a case for every G.
  * the capped grid: m = slice * (parts + 3) + 5 with parts, the step kernel's workgroup count at saturation, read from the workspace query
    (never restated here).  Slices parts .. parts + 3 are second turns of workgroups 0 .. 3.  Planted winners: in a second-turn slice; in a
    slice >= 1024 (the pick kernel's second pass over the parts); the last item; two exact ties whose smaller id must win -- one against a
    larger id in a LOWER-numbered workgroup, one against a larger id that the SAME thread meets on its second turn; a NaN column in a
    second-turn slice.
Generic data (pn.GENERIC_LARGE, fp32 and bf16) against the numpy restatement: its minimum gap is asserted >= 2^-30 first (a condition on the
reference alone; measured 2^-11.2 .. 2^-18.0 on these inputs), then ids for equality and |gain_dev - gain_ref| <= 16 (kq + 4 k) 2^-53 d_first:
the derivation of the older file with its 16-fold margin, written from the sizes (the measured maxima are in DESIGN 4.4f).

Mutations tried on scratch builds when this file was written (each only drops work; the whole of tests/test_gpu_select_pivoted.py PASSES on
every one of them -- that is the gap this file closes):
  * pivot_pick_kernel's G == 1 update runs its first pass only (rows from 1024 on keep their component along the basis): the generic cases
    kq = 1027 and kq = 4096 fail, fp32 and bf16 (4 tests, ids differ).  The exact cases at kq = 1027 and 4096 pass: see above.
  * pivot_pick_kernel's loop over the parts runs its first pass only: test_capped_grid... fails, fp32 and bf16 (the winner planted in slice
    1500 is never seen).
  * pivot_step_kernel's slice loop becomes an `if`: test_capped_grid... fails, fp32 and bf16 (the second-turn slices keep the poison in d).
A fourth, which the older file does catch at its G = 8 and 16 -- the last group's share of the G > 1 update dropped -- fails the generic cases
kq = 256, 320 and 512 here (G = 4, 3, 2; 6 tests) and none of the exact ones.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pivot_numpy as pn  # noqa: E402
from test_gpu_select_pivoted import DTYPES, _poisoned, _raw, _scales  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _select_poisoned(ops, R, k):
	"""anncur_select_pivoted on R with every byte of the outputs and of a private workspace 0xff -> (ids int64 [k], gains [k], n_sel); nothing is
	written past position k of the outputs or past n_sel's word."""
	from anncur_amd import _lib
	lib = _lib.load()
	kq, m = R.shape
	assert R.stride(1) == 1
	ids, gains, n_sel, ws = _poisoned(k, lib.anncur_select_pivoted_workspace_bytes(m, kq, k))
	assert _raw(lib, R.data_ptr(), ops._DT[R.dtype], R.stride(0), kq, m, k, ids, gains, n_sel, ws) == 0
	torch.cuda.synchronize()
	assert n_sel[1:].tolist() == [-1, -1] and ids[k:].tolist() == [-1, -1] and gains[k:].view(torch.int64).tolist() == [-1, -1]
	return ids[:k].cpu().numpy().astype(np.int64), gains[:k].cpu().numpy(), int(n_sel[0].item())


def _device_items(scales, kq, n, dtype):
	R = torch.from_numpy(pn.hadamard_items(scales, kq, n=n).astype(np.float32)).cuda().to(DTYPES[dtype])
	return R


# ------------------------------------------------------------------ exact data at every shape of the pick kernel
# (n, kq, k): what the shape reaches is in the module docstring
PICK_SHAPES = [(256, 256, 40), (256, 320, 40), (256, 512, 40), (256, 603, 40), (1024, 1027, 40), (4096, 4096, 24)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n, kq, k", PICK_SHAPES, ids=[f"n{n}-kq{kq}" for n, kq, _ in PICK_SHAPES])
def test_exact_at_every_shape_of_the_pick_kernel(ops, n, kq, k, dtype):
	"""Three full slices and a tail of 5 items, |s| <= 9 (exact in bf16), k above the 16 waves of the coefficient loop.  With 9 values of s^2 on
	k picks the gains tie exactly, many times over; from step 1 on every Gram-Schmidt coefficient is an exact 0 and q_t = +-1/sqrt(n)."""
	m = 3 * ops.select_pivoted_slice_items(DTYPES[dtype]) + 5
	scales = _scales(m, seed=kq)
	want_ids, want_gains, want_n = pn.hadamard_closed_form(scales, k, n=n)
	assert want_n == k and len(set(want_gains.tolist())) < k
	ids, gains, n_sel = _select_poisoned(ops, _device_items(scales, kq, n, dtype), k)
	assert n_sel == want_n
	assert np.array_equal(ids, want_ids), (ids, want_ids)
	assert np.array_equal(gains, want_gains)


# ------------------------------------------------------------------ the capped grid
def _saturated_parts(lib, kq, k):
	"""The step kernel's workgroup count once its grid is capped, from the workspace query: header, d[m], basis [k x kq], 16 bytes per part."""
	from anncur_amd import _lib
	up256 = lambda b: (b + 255) & ~255
	parts_at = lambda m: (lib.anncur_select_pivoted_workspace_bytes(m, kq, k) - 256 - up256(8 * m) - up256(8 * k * kq)) // 16
	m = 1 << 22
	parts = parts_at(m)
	assert parts == parts_at(2 * m) and parts > 0                 # saturated
	assert parts < -(-m // lib.anncur_select_pivoted_slice_items(_lib.F32))   # ... and below the slice count: a cap, not the count
	return int(parts)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_capped_grid_second_turn_slices_and_ties_across_turns(ops, dtype):
	from anncur_amd import _lib
	lib = _lib.load()
	n = kq = k = 16
	parts = _saturated_parts(lib, kq, k)
	S = ops.select_pivoted_slice_items(DTYPES[dtype])
	assert S % 16 == 0 and parts > 1024 + 476
	m = S * (parts + 3) + 5                                       # slices 0 .. parts + 2 full, slice parts + 3 = the tail of 5 items
	scales = _scales(m, seed=16)
	at = lambda sl, off: sl * S + off                             # (S % 16 == 0: the direction of an item is its offset mod 16)
	second_turn = at(parts + 1, 32)                               # 1. direction 0, a slice that workgroup 1 takes on its second turn
	far_part = at(1024 + 476, 17)                                 # 2. direction 1, workgroup 1500: the pick kernel's second pass over the parts
	last = m - 1                                                  # 3. direction 4, the ragged tail (workgroup 3's second turn)
	tie_a, tie_a_loser = at(7, 18), at(parts + 3, 2)              # 4. direction 2: the smaller id in workgroup 7, the larger in workgroup 3
	tie_b, tie_b_loser = at(2, 51), at(parts + 2, 51)             # 5. direction 3: one thread of workgroup 2 meets both, the smaller id first
	nan_col = at(parts + 1, 22)                                   # 6. direction 6: would be the first pick; its column is NaN
	assert [i % 16 for i in (second_turn, far_part, last, tie_a, tie_a_loser, tie_b, tie_b_loser, nan_col)] == [0, 1, 4, 2, 2, 3, 3, 6]
	assert tie_a < tie_a_loser < m and tie_b < tie_b_loser and (parts + 1) * S <= nan_col < m
	for i, s in ((second_turn, 100), (far_part, 99), (last, 98), (tie_a, 97), (tie_a_loser, -97), (tie_b, -96), (tie_b_loser, 96), (nan_col, 120)):
		scales[i] = s                                             # (|s| <= 256: exact in bf16)
	R = _device_items(scales, kq, n, dtype)
	R[:, nan_col] = float("nan")
	want_ids, want_gains, want_n = pn.hadamard_closed_form(scales, k, never=(nan_col,), n=n)
	assert want_n == 16
	ids, gains, n_sel = _select_poisoned(ops, R, k)
	assert list(ids[:5]) == [second_turn, far_part, last, tie_a, tie_b], ids
	assert list(gains[:5]) == [16.0 * s * s for s in (100, 99, 98, 97, 96)]
	assert n_sel == want_n and nan_col not in ids
	assert np.array_equal(ids, want_ids), (ids, want_ids)
	assert np.array_equal(gains, want_gains)
	assert (gains[5:] == 16.0 * 81).all()                         # the other eleven directions tie at |s| = 9: the smallest id of each, in id order
	assert (np.diff(ids[5:]) > 0).all()


# ------------------------------------------------------------------ generic data at large kq against the restatement
@functools.lru_cache(maxsize=None)
def _generic_large(case, dtype):
	kq, m, k, rank, noise, seed = pn.GENERIC_LARGE[case]
	R = torch.from_numpy(pn.low_rank(kq, m, rank, noise, seed))
	if dtype == "bf16":
		R = R.bfloat16()
	ref = pn.select(R.float().numpy(), k)                        # the reference sees the values the device sees
	return R.cuda(), k, ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(pn.GENERIC_LARGE)), ids=[f"kq{c[0]}-m{c[1]}" for c in pn.GENERIC_LARGE])
def test_generic_data_at_large_kq_equals_the_restatement(ops, case, dtype):
	R, k, (want_ids, want_gains, want_n, gaps) = _generic_large(case, dtype)
	kq = R.shape[0]
	print(f"{tuple(R.shape)} {dtype}, k = {k}: minimum gap of the restatement 2^{np.log2(gaps.min()):.1f}")
	assert want_n == k and gaps.min() >= 2.0 ** -30               # a condition on the reference alone
	ids, gains, n_sel = _select_poisoned(ops, R, k)
	assert n_sel == k and np.array_equal(ids, want_ids), (ids, want_ids)
	bound = 16.0 * (kq + 4 * k) * 2.0 ** -53 * want_gains[0]
	err = np.abs(gains - want_gains).max()
	print(f"  max |gain_dev - gain_ref| = {err:.3g} = 2^{np.log2(max(err, 1e-300) / want_gains[0]):.1f} d_first, bound {bound:.3g} = 2^{np.log2(bound / want_gains[0]):.1f} d_first")
	assert err <= bound
	assert (np.diff(gains) <= bound).all()                        # non-increasing up to the same bound
