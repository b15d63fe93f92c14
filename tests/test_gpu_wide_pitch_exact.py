"""Exact-data tests with a row pitch beyond the kernels' 32-bit tile offsets (DESIGN "Operands beyond 32-bit offsets", regime 2): a
256-row block whose row 255 lies more than 2^32 bytes behind its row 0.  300 rows, so that row 255 of a row block exists, at a pitch of
8.6 M elements (tests/far_layouts.py wide_pitch: 5.2 GB of bf16, 0xff poison between the rows).  Small-integer operands: every result must
be bit-equal to the compact twin's AND to a host reference.

  - wide_kernel (csrc/score_wide.hpp) addresses its query rows as a 64-bit block base + a 32-bit byte offset; from a query pitch of
    8 421 512 elements on, the offsets of the last rows of a block wrap and the prepass and the sweep read other queries (or the poison), inside
    the allocation and silently.  anncur_score_topk now refuses such a call (wide_query_offsets_fit) and ops.score_topk_fused / ops.eval_topk
    pass a compact copy of the queries.  ON THE PARENT COMMIT test_fused_wide_route_with_a_far_query_pitch FAILS (both Kp, both entry points).
    (At 8.6 M the offsets of rows 250..255 of a block wrap; at the first refused pitch, 8 421 512, row 255's.)
  - ivf_tile128_kernel (csrc/ivf.hip) forms query and vector addresses as 32-bit byte offsets; ivf_use_tile128 takes it only while
    nq x ldq x 2 < 2^32 and 128 x ldx x 2 < 2^32.  Both halves of the gate, on both sides, against the host search.
  - the exact-matrix twin of the first item (error_lds_kernel / evalf_kernel) is
    tests/test_gpu_kernels.py::test_error_kernels_with_a_row_pitch_beyond_the_32_bit_tile_offsets, left where it is.

The fused cases fill the buffer with a finite decoy (1.0) instead of the NaN poison, and compare the number of queries the select had to
repair with the compact twin's: a query row read from NaN ends without candidates and is recomputed by the select's repair path (its own
64-bit addressing) -- on the code before the gate, six fallbacks and the right top-k.  A column slice of a real matrix holds finite numbers
there, and the answer is then silently wrong.

Mutation tried on a scratch build (never committed): the parent commit's library and ops.py, i.e. no gate and no compact copy.  The wrapped
offsets stay inside the 5.2 GB buffer (an unsigned wrap of a byte offset below 300 x pitch x 2 lands in the body), so the run is safe.
All four cases of test_fused_wide_route_with_a_far_query_pitch fail; the IVF cases pass.  (7 tests, 2.2 s on an MI355X.)
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_layouts as fl  # noqa: E402
import fused_exact_cases as fx  # noqa: E402
from ivf_index_numpy import lists_search_ref  # noqa: E402

pytestmark = pytest.mark.gpu
Q = 300
PITCH = 8_600_000
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@pytest.fixture(scope="module")
def xwide(ops):
	"""One [300 x 1024] bf16 view at the far pitch and its buffer, shared by the fused cases (each refills it and writes its own columns)."""
	view, buf = fl.wide_pitch(Q, 1024, BF16, "cuda", PITCH)
	yield view, buf
	del view, buf
	torch.cuda.empty_cache()


def _same(a, b):
	return torch.equal(fx.bits(a.values), fx.bits(b.values)) and torch.equal(a.indices, b.indices)


@pytest.mark.parametrize("entry", ["score_topk_fused", "eval_topk"])
@pytest.mark.parametrize("Kp,K", [(640, 513), (1024, 900)])
def test_fused_wide_route_with_a_far_query_pitch(ops, xwide, Kp, K, entry):
	from anncur_amd import _lib
	I, k = 8203, 100
	assert ops.fused_plan(Q, I, Kp, k)["lg"] == 4
	xwide, xbuf = xwide
	X, E, S = fx.dense_case(Q, I, K, seed=Kp)
	Xc, Etp = fx.device_operands(ops, X, E, Kp)
	# A finite decoy between the rows instead of the NaN poison: the select REPAIRS a query that ends without candidates, so a query row read
	# from NaN is recomputed by the repair path and comes out right (seen on the code before the gate: 6 fallbacks, the right top-k) -- a
	# finite wrong row comes out wrong, as a column slice of a real matrix would.
	xbuf.fill_(1.0)
	Xw = xwide[:, :Kp]
	Xw.copy_(Xc)
	assert Xw.stride(0) == PITCH and 255 * PITCH * 2 >= 1 << 32
	want_v, want_rows = fx.reference_topk(S, k)
	if entry == "score_topk_fused":
		ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
		far, nfb_far = ops.score_topk_fused(Xw, Etp, I, k, workspace=ws, return_fallbacks=True)
		nfb_far = int(nfb_far[0].item())
		ws.fill_(0xff)
		near, nfb_near = ops.score_topk_fused(Xc, Etp, I, k, workspace=ws, return_fallbacks=True)
		assert nfb_far == int(nfb_near[0].item()), "queries repaired by the select differ between the far pitch and the compact twin"
		# the C entry point itself refuses the pitched operand, with the limit in its message, before it launches anything
		rc = _lib.load().anncur_score_topk_ex(ops._p(Xw), PITCH, ops._p(Etp), Kp, Q, I, Kp, k, ops._p(far.values), ops._p(far.indices), ops._p(ws), ws.numel(), 0, None, None)
		assert rc != 0 and b"too long for the wide kernel's 32-bit row offsets" in _lib.load().anncur_last_error()
	else:
		g = torch.Generator().manual_seed(Kp)
		A = torch.randint(-100, 101, (Q, I), generator=g, dtype=torch.int32)
		Ad = A.to(BF16).cuda()
		(ex_far, far), (ex_near, near) = ops.eval_topk(Ad, 10, Xw, Etp, I, k), ops.eval_topk(Ad, 10, Xc, Etp, I, k)
		ev, ei = fx.reference_topk(A, 10)
		for ex in (ex_far, ex_near):
			assert torch.equal(ex.values.cpu().double(), ev.double()) and torch.equal(ex.indices.cpu().long(), ei)
	torch.cuda.synchronize()
	for name, got in (("compact", near), ("far pitch", far)):
		bad = ((got.values.cpu().double() != want_v.double()) | (got.indices.cpu().long() != want_rows)).any(1).nonzero()[:, 0]
		assert bad.numel() == 0, f"{name}: {bad.numel()} queries differ from the host top-k, first {bad[:8].tolist()}"
	assert _same(far, near)
	assert torch.equal(Xw, Xc)                                         # (the operand is read only)


# ------------------------------------------------------------------ IVF: both halves of the tile-128 gate
def _ivf_case(nq, sizes, dp=128, nprobe=3, seed=0):
	g = np.random.default_rng(seed)
	sizes = np.asarray(sizes, dtype=np.int64)
	n, nlist = int(sizes.sum()), sizes.shape[0]
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X = g.integers(-8, 9, (n, dp)).astype(np.int64)
	Qh = g.integers(-8, 9, (nq, dp)).astype(np.int64)
	probe = g.integers(0, nlist, (nq, nprobe)).astype(np.int32)
	probe[::7, 1] = -1                                                   # holes
	return sizes, off, ids, X, Qh, probe


def _search(ops, Xd, Qd, off, ids, sizes, probe, k, want_tile):
	from anncur_amd import _lib
	assert _lib.load().anncur_ivf_search_tile(ops._dt(Xd), Xd.shape[1], ops._ld(Xd), ops._ld(Qd), Qd.shape[0]) == want_tile
	for cls, v in ((ops._ScoreScratch, float("inf")), (ops._ByteScratch, 0xff)):
		for b in cls._bufs.values(): b.fill_(v)
	got = ops.ivf_search_grouped(Xd, torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda(), sizes, Qd, torch.from_numpy(probe).cuda(), k)
	torch.cuda.synchronize()
	return got


def _ivf_equal(got, want, what):
	gv, gi = got.values.cpu(), got.indices.cpu().to(torch.int32)
	bad = ((gv != torch.from_numpy(want[0])) | (gi != torch.from_numpy(want[1]))).any(1).nonzero()[:, 0]
	assert bad.numel() == 0, f"{what}: {bad.numel()} queries differ, first {bad[:8].tolist()}"


@pytest.mark.parametrize("ldx,tile", [((1 << 24) - 8, 128), (1 << 24, 64)], ids=["below", "at"])
def test_ivf_search_vector_pitch_on_both_sides_of_the_tile128_gate(ops, ldx, tile):
	"""128 x ldx x 2 = 2^32 at ldx = 16 777 216: 300 rows (10 GB of bf16).  k = 128 and every query probes at most 128 vectors -- the one list
	that fills a 128-vector tile (row 127 of a tile: the largest offset the gate is about) alone, or three short lists --, so EVERY probed
	vector's score is in the result: a vector row read from the poison scores NaN and would silently leave a top-10."""
	sizes, off, ids, X, Qh, probe = _ivf_case(40, [128, 0, 1, 42, 40, 39, 50], seed=1)     # (300 vectors; the last list is never probed)
	probe[:, :] = 1 + (probe % 5)
	probe[::3] = [0, -1, -1]
	k = 128
	want = lists_search_ref(X, Qh, off, ids, probe, k, ("packed",))["packed"]
	Xc, Qc = torch.from_numpy(X).to(BF16).cuda(), torch.from_numpy(Qh).to(BF16).cuda()
	Xw, buf = fl.wide_pitch(300, 128, BF16, "cuda", ldx)
	try:
		Xw.copy_(Xc)
		far = _search(ops, Xw, Qc, off, ids, sizes, probe, k, tile)
		near = _search(ops, Xc, Qc, off, ids, sizes, probe, k, 128)
		_ivf_equal(near, want, "compact")
		_ivf_equal(far, want, f"ldx = {ldx}")
		assert _same(far, near)
	finally:
		del Xw, buf
		torch.cuda.empty_cache()


def test_ivf_search_query_pitch_on_both_sides_of_the_tile128_gate(ops):
	"""nq x ldq x 2 crosses 2^32 between nq = 249 and nq = 250 at ldq = 8.6 M; nq = 300 has a query row 255 and beyond."""
	sizes, off, ids, X, Qh, probe = _ivf_case(Q, [129, 0, 1, 128, 300, 42], seed=2)
	k = 10
	want = lists_search_ref(X, Qh, off, ids, probe, k, ("packed",))["packed"]
	Xc, Qc = torch.from_numpy(X).to(BF16).cuda(), torch.from_numpy(Qh).to(BF16).cuda()
	Qw, buf = fl.wide_pitch(Q, 128, BF16, "cuda", PITCH)
	try:
		Qw.copy_(Qc)
		for nq, tile in ((249, 128), (250, 64), (300, 64)):
			far = _search(ops, Xc, Qw[:nq], off, ids, sizes, probe[:nq], k, tile)
			near = _search(ops, Xc, Qc[:nq], off, ids, sizes, probe[:nq], k, 128)
			_ivf_equal(near, (want[0][:nq], want[1][:nq]), f"compact nq = {nq}")
			_ivf_equal(far, (want[0][:nq], want[1][:nq]), f"ldq = {PITCH}, nq = {nq}")
			assert _same(far, near)
	finally:
		del Qw, buf
		torch.cuda.empty_cache()
