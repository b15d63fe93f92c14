"""Exact-data tests with operand rows beyond 2^31 and 2^32 elements (DESIGN "Operands beyond 32-bit offsets", regime 1).

Every case runs an entry point on a FAR view (tests/far_layouts.py far_rows: a front guard of 2^31 poisoned elements, then rows whose starts
lie below 2^31, in [2^31, 2^32) and at or beyond 2^32 elements from the view's first element; 0xff poison everywhere else) and on the view's
compact copy.  The data are small integers, so every sum is exact in any order: the two results must be bit-equal to each other AND to a
host reference of the operation (tests/topk_numpy.py, rank_numpy.py, gumbel_numpy.py, pivot_numpy.py, ivf_index_numpy.py,
fused_exact_cases.py, or plain integer numpy).  No tolerances.  Every row carries its own random data, so a kernel that forms
row x pitch in 32 bits reads another row or the poison (NaN / a hole) and fails instead of faulting; where the far operand is an output,
far_layouts.assert_only_view_written compares the whole allocation outside the view with the poison afterwards.

One slot holds an fp32 / int32 far buffer (24 GiB), one a 16-bit one (12 GiB); a test that needs another layout frees the slot's buffer
first (_far), and the module frees both at its end.  Section 3 builds item matrices of more than 2^31 elements (4.3 GB) on the device and
plants the winners, so its reference is known by construction.

Two ways in which a wrong read can hide, and what the cases do about them:
  - the fused top-k's select REPAIRS a query that ends without candidates, so a query row read from NaN poison is recomputed by the repair
    path and comes out right.  The fused cases therefore fill the allocation with a finite decoy (1.0) instead, and compare the number of
    repaired queries with the compact twin's;
  - a far ITEM row (IVF vectors, rescore's Et) read from the poison scores NaN and silently leaves a top-k it was not part of anyway.  The
    IVF cases plant the winners in the far rows; rescore_topk returns every candidate.

Not covered: the fp32 far-QUERY case of ivf_search_grouped reaches element 2^31 + 16 (byte 2^33 + 64) only, no row at or beyond 2^32
elements -- beside 24 GiB of fp32 vectors the queries live in the 16-bit slot's 12 GiB seen as fp32 (the memory budget above).

Mutations tried on scratch builds when this file was written (never committed).  Only mutants whose wrapped
address provably stays inside the guarded allocation were run -- that is what the guard is for:
  * gather_cols_kernel with `A + (int)(r * lda)` (rows 2 and 3 land in the guard, row 4 in the body): test_rerank_gather_pairs_and_gather_cols
    fails for both dtypes; the row scans (test_rowwise_topk), run beside it as a control, pass.
  * ivf_scan_kernel with `(uint32_t)` on the vector row offset (row 2999 lands in the poison behind row 0):
    test_ivf_list_means_and_scan_with_far_vectors fails (on random vectors with k = 10 it survives: the one wrapped vector scores NaN and is
    in no top-10 -- hence the planted winners).
  * lstsq_matvec_kernel with `Rt[(uint32_t)(id * ldr) + a]` (item row 66 lands in the poison behind row 0): test_lstsq_rows_with_far_operands[Rt]
    fails; [ids_C] and select_pivoted, run beside it, pass.
  * the wide route's new gate dropped: see tests/test_gpu_wide_pitch_exact.py.

Needs an MI355X with 48 GiB free."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_layouts as fl  # noqa: E402
import fused_exact_cases as fx  # noqa: E402
import gumbel_numpy as gn  # noqa: E402
import ivf_index_numpy as ivfn  # noqa: E402
import pivot_numpy as pn  # noqa: E402
from rank_numpy import rank_ref  # noqa: E402
from topk_numpy import rerank_ref, topk_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
BOTH = ["bf16", "f32"]
WIDTH = {5: 8192, 67: 4104, 3000: 128}    # columns of the far view per row count (a test takes the leading columns it needs)
I_ROW = 4099                               # row length of the score-matrix cases: 512 vectors of 8 and a ragged tail of 3
_SLOT = {}


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	yield _ops
	_SLOT.clear()
	torch.cuda.empty_cache()


def _far(rows, dtype, misalign=0, slot=None, decoy=None):
	"""(poisoned far view [rows x WIDTH[rows]], its buffer): one fp32-sized and one 16-bit layout alive at a time.  slot: put a 16-bit layout
	into the fp32 slot (a second 12 GiB buffer instead of a 24 GiB one).  decoy: fill the WHOLE allocation with this finite value instead of
	the poison -- for the fused top-k, whose select repairs a query that ends without candidates: a query row read from NaN poison would be
	recomputed by the repair path and come out right; a finite wrong row comes out wrong.  The next fetch poisons the allocation again."""
	slot = slot or ("f32" if torch.empty((), dtype=dtype).element_size() == 4 else "other")
	key = (rows, dtype, misalign)
	cur = _SLOT.get(slot)
	if cur is None or cur[0] != key:
		_SLOT.pop(slot, None)
		cur = None
		torch.cuda.empty_cache()
		view, buf = fl.far_rows(rows, WIDTH[rows], dtype, "cuda", misalign)
		off = [r * view.stride(0) for r in range(rows)]
		assert any(1 << 31 <= o < 1 << 32 for o in off) and off[-1] >= 1 << 32
		_SLOT[slot] = cur = [key, view, buf, False]
	if cur[3]:
		cur[2].view(torch.int64).fill_(-1)
		cur[3] = False
	if decoy is not None:
		cur[2].fill_(decoy)
		cur[3] = True
	else:
		fl.repoison(cur[1])
	return cur[1], cur[2]


def _ints(rows, cols, lim, seed, lo=None):
	g = torch.Generator().manual_seed(seed)
	return torch.randint(-lim if lo is None else lo, lim + 1, (rows, cols), generator=g)


def _put(H, dtype, misalign=0):
	"""Host integers H [rows x cols] -> (far view holding them, compact device copy, the far buffer)."""
	view, buf = _far(H.shape[0], dtype, misalign)
	rows, cols = H.shape
	if misalign:
		near = H.to(dtype).cuda()
	else:   # the compact twin's rows are 16-byte aligned too (pitch rounded up to 8, NaN in the pad): the same vector paths on both sides
		near = torch.full((rows, -(-cols // 8) * 8), float("nan"), dtype=dtype, device="cuda")[:, :cols]
		near.copy_(H.to(dtype))
	far = view[:, :H.shape[1]]
	far.copy_(near)
	assert far.stride(0) == view.stride(0) >= 1 << 20 and torch.equal(far, near)
	return far, near, buf


def _eq(got, want, what):
	"""Bit equality of a device result with a host array (NaN patterns compare as bits of the fp32 view where the dtype is fp32)."""
	g = got.detach().cpu()
	w = torch.as_tensor(np.asarray(want)) if not torch.is_tensor(want) else want
	assert g.shape == w.shape, (what, g.shape, w.shape)
	if g.dtype == torch.float32:
		ok = (g.view(torch.int32) == w.to(torch.float32).view(torch.int32)) | (g.isnan() & w.to(torch.float32).isnan())
	else:
		ok = g.to(torch.int64) == w.to(torch.int64) if not g.dtype.is_floating_point else g.double() == w.double()
	bad = (~ok).nonzero()
	assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def _both(what, fn, far, near, *want):
	"""fn(operand) on the far view and on the compact copy: each result tensor against the host reference."""
	for name, A in (("compact", near), ("far", far)):
		got = fn(A)
		got = got if isinstance(got, (tuple, list)) else (got,)
		torch.cuda.synchronize()
		assert len(got) >= len(want)
		for j, w in enumerate(want):
			_eq(got[j], w, f"{what} [{name}] result {j}")


# ================================================================== 1. score-matrix rows (lda / lds)
@pytest.mark.parametrize("misalign", [0, 3])
@pytest.mark.parametrize("k", [1, 128])
@pytest.mark.parametrize("dt", BOTH)
def test_rowwise_topk(ops, dt, k, misalign):
	H = _ints(5, I_ROW, 120, 1)
	far, near, _ = _put(H, DT[dt], misalign)
	ref = [topk_ref(H[q].numpy(), k) for q in range(5)]
	_both("rowwise_topk", lambda A: tuple(ops.rowwise_topk(A, k)), far, near, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))


@pytest.mark.parametrize("dt", BOTH)
def test_rowwise_topk_ragged_and_gather(ops, dt):
	H = _ints(5, I_ROW, 120, 2)
	far, near, _ = _put(H, DT[dt])
	k = 16
	lens = [k, I_ROW, 1000, 2049, 17]
	row_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
	ref = [topk_ref(H[q, :lens[q]].numpy(), k) for q in range(5)]
	_both("rowwise_topk_ragged", lambda A: tuple(ops.rowwise_topk_ragged(A, row_len, k)), far, near, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
	cols = torch.tensor([0, 7, 8, 1000, 2048, 4090, I_ROW - 1], dtype=torch.int32, device="cuda")
	tables = ops.gather_tables(cols, I_ROW, DT[dt])
	ref = [topk_ref(H[q].numpy(), k) for q in range(5)]

	def call(A):
		top, cq = ops.rowwise_topk_gather(A, k, tables)
		return top.values, top.indices, cq.float()
	want = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), H[:, cols.cpu().long()].float())
	_both("rowwise_topk_gather", call, far, near, *want)
	# cq_out (ldo) far: in the same allocation as A, behind its columns (one pitch) -- and alone, A compact, with the whole-allocation check
	view, buf = _SLOT["f32" if dt == "f32" else "other"][1:3]
	cq = buf.as_strided((5, cols.numel()), (view.stride(0), 1), view.storage_offset() + 4104)
	top, _ = ops.rowwise_topk_gather(far, k, tables, cq_out=cq)
	torch.cuda.synchronize()
	for j, g in enumerate((top.values, top.indices, cq.float())):
		_eq(g, want[j], f"rowwise_topk_gather, A and cq_out far, result {j}")
	assert torch.equal(far, near) and (fl._int_alias(view[:, I_ROW:4104]) == -1).all() and (fl._int_alias(view[:, 4104 + cols.numel():]) == -1).all()
	view, buf = _far(5, DT[dt])
	cq = view[:, :cols.numel()]
	top, _ = ops.rowwise_topk_gather(near, k, tables, cq_out=cq)
	torch.cuda.synchronize()
	got = cq.clone()
	fl.assert_only_view_written(buf, cq)
	for j, g in enumerate((top.values, top.indices, got.float())):
		_eq(g, want[j], f"rowwise_topk_gather, cq_out far, result {j}")


@pytest.mark.parametrize("dt", BOTH)
def test_rerank_gather_pairs_and_gather_cols(ops, dt):
	H = _ints(5, I_ROW, 120, 3)
	far, near, _ = _put(H, DT[dt])
	g = torch.Generator().manual_seed(3)
	cand = torch.stack([torch.randperm(I_ROW - 1, generator=g)[:50] for _ in range(5)]).int()   # distinct
	cand[:, 0] = I_ROW - 1
	ref = [rerank_ref(H[q].numpy(), cand[q].numpy(), 10) for q in range(5)]
	cd = cand.cuda()
	_both("rerank", lambda A: tuple(ops.rerank(A, cd, 50, 10)), far, near, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
	pairs = cand[:, :33].clone()
	pairs[:, 5], pairs[:, 6] = -1, I_ROW                                  # holes
	hole = (pairs < 0) | (pairs >= I_ROW)
	want = torch.where(hole, torch.tensor(float("nan")), torch.gather(H, 1, pairs.clamp(0, I_ROW - 1).long()).float())
	pd = pairs.cuda()
	_both("gather_pairs", lambda A: ops.gather_pairs(A, pd), far, near, want)
	idx = [0, 1, 7, 8, 4090, I_ROW - 1, 2048, 2048]
	_both("gather_cols", lambda A: ops.gather_cols(A, idx).float(), far, near, H[:, idx].float())
	_both("gather_cols to fp32", lambda A: ops.gather_cols(A, idx, out_dtype=torch.float32), far, near, H[:, idx].float())


@pytest.mark.parametrize("misalign", [0, 3])
@pytest.mark.parametrize("dt", BOTH)
def test_rank_in_rows(ops, dt, misalign):
	H = _ints(5, I_ROW, 60, 4)                                            # narrow range: ties everywhere
	far, near, _ = _put(H, DT[dt], misalign)
	g = torch.Generator().manual_seed(4)
	ids = torch.randint(0, I_ROW, (5, 9), generator=g, dtype=torch.int32)
	ids[:, 0], ids[:, 1], ids[:, 2] = 0, I_ROW - 1, -1
	want_rank = rank_ref(H.float().numpy(), ids.numpy())
	want_score = torch.where(ids < 0, torch.tensor(float("nan")), torch.gather(H, 1, ids.clamp(min=0).long()).float())
	_both("rank_in_rows", lambda A: ops.rank_in_rows(A, ids, return_scores=True), far, near, want_rank, want_score)


def test_sample_topk(ops):
	H = _ints(5, I_ROW, 8, 5)
	far, near, _ = _put(H, torch.float32)
	k, seed, stream = 16, 11, 2
	G = ops.gumbel_noise(seed, stream, 5, I_ROW).cpu().numpy()
	want_k, want_i = gn.sample_reference(H.float().numpy(), 1.0, G, k)
	_both("sample_topk", lambda A: tuple(ops.sample_topk(A, k, 1.0, seed, stream)), far, near, want_k, want_i)


@pytest.mark.parametrize("dt", BOTH)
def test_gather_rows_over_67_far_rows(ops, dt):
	H = _ints(67, 1003, 120, 6)
	far, near, _ = _put(H, DT[dt])
	off = [r * far.stride(0) for r in range(67)]
	ids = [0, 66, 33, 32, 65, 34, 1, 66]                                  # rows on both sides of 2^31 (row 33) and of 2^32 (row 66)
	assert off[32] < 1 << 31 <= off[33] and off[65] < 1 << 32 <= off[66]
	_both("gather_rows", lambda A: ops.gather_rows(A, ids).float(), far, near, H[ids].float())


@pytest.mark.parametrize("src_far,dst_far", [(True, False), (False, True), (True, True)], ids=["src", "dst", "both"])
@pytest.mark.parametrize("s,d", [("bf16", "f32"), ("f32", "bf16")])
def test_convert(ops, s, d, src_far, dst_far):
	from anncur_amd import _lib
	H = _ints(5, I_ROW, 120, 7)
	far, near, _ = _put(H, DT[s])
	src = far if src_far else near
	if not dst_far:
		_eq(ops.convert(src, DT[d]), H.to(DT[d]).float() if d == "bf16" else H.float(), "convert")
		return
	view, buf = _far(5, DT[d])
	dst = view[:, :I_ROW]
	_lib.check(_lib.load().anncur_convert(ops._p(src), ops._dt(src), ops._ld(src), ops._p(dst), ops._dt(dst), dst.stride(0), 5, I_ROW, ops._stream()), "convert")
	torch.cuda.synchronize()
	got = dst.clone()
	fl.assert_only_view_written(buf, dst)
	_eq(got.float(), H.float(), "convert into a far destination")


def test_pack_bf16_and_pack_split(ops):
	K = 300
	H = _ints(5, K, 40000, 8)                                             # 17-bit integers: hi = bf16(x) and lo = x - hi, both exact
	far, near, _ = _put(H, torch.float32)
	small = (H % 97 - 48)
	hi = H.float().bfloat16().float()
	lo = (H.float() - hi).bfloat16().float()
	assert torch.equal(lo, H.float() - hi) and lo.abs().max() > 0
	Kp = ops.split_kp(K)
	z = torch.zeros(5, Kp - 3 * K)
	_both("pack_split_bf16 role 0", lambda A: ops.pack_split_bf16(A, 0).float(), far, near, torch.cat([lo, hi, hi, z], 1))
	_both("pack_split_bf16 role 1", lambda A: ops.pack_split_bf16(A, 1).float(), far, near, torch.cat([hi, lo, hi, z], 1))
	far.copy_(small.float().cuda())
	want = torch.zeros(5, 512)
	want[:, :K] = small.float()
	_both("pack_bf16", lambda A: ops.pack_bf16(A, 512).float(), far, small.float().cuda(), want)


def test_sumsq_and_scale_copy(ops):
	H = _ints(5, I_ROW, 20, 9)
	far, near, buf = _put(H, torch.float32)
	total = float((H * H).sum())
	assert total < 1 << 24
	_both("sumsq ordered", lambda A: ops.sumsq(A), far, near, np.array([total], dtype=np.float32))
	_both("sumsq", lambda A: ops.sumsq(A, ordered=False), far, near, np.array([total], dtype=np.float32))
	out = torch.full((5, I_ROW), float("nan"), device="cuda")
	_eq(ops.scale_copy(far, out, alpha=2.0), 2.0 * H.float(), "scale_copy from far rows")
	view, buf = _far(5, torch.float32)
	dst = view[:, :I_ROW]
	ops.scale_copy(near, dst, alpha=-2.0)
	torch.cuda.synchronize()
	got = dst.clone()
	fl.assert_only_view_written(buf, dst)
	_eq(got, -2.0 * H.float(), "scale_copy into far rows")


@pytest.mark.parametrize("dt", BOTH)
def test_approx_error_with_a_far_exact_matrix(ops, dt):
	K = 8
	g = torch.Generator().manual_seed(10)
	X = torch.randint(0, 3, (5, K), generator=g)
	E = torch.randint(-2, 3, (I_ROW, K), generator=g)
	A = _ints(5, I_ROW, 20, 10)
	S = X @ E.t()
	err, nrm = ((S - A) ** 2).sum(1), (A * A).sum(1)
	assert int(err.max()) < 1 << 24
	far, near, _ = _put(A, DT[dt])
	Xd, Ed = X.float().cuda(), E.float().cuda()
	_both("approx_error", lambda M: ops.approx_error(Xd, Ed, M), far, near, err.float(), nrm.float())
	Xp, Etp = ops.pack_bf16(Xd, 64), ops.pack_bf16(Ed, 64, row_multiple=32)
	assert ops.approx_error_packed_ok(64, far)
	_both("approx_error_packed", lambda M: ops.approx_error_packed(Xp, Etp, M, I_ROW), far, near, err.float(), nrm.float())


def test_norm_buckets_and_renorm_rows(ops):
	from anncur_amd import _lib
	H = _ints(67, 300, 8, 11)
	H[5] = 0
	far, near, buf = _put(H, torch.float32)

	def buckets(M):
		n = M.shape[0]
		norms, mm, b = torch.empty(n, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
		_lib.check(_lib.load().anncur_norm_buckets(ops._p(M), n, M.shape[1], ops._ld(M), 16, ops._p(norms), ops._p(mm), ops._p(b), ops._stream()), "norm_buckets")
		return norms, b
	want_norms = (H * H).sum(1).float()
	f = np.float32                                                       # norm_bucket_kernel's formula, one IEEE fp32 operation per step (as tests/test_gpu_ivf_exact.py restates it)
	nv = want_norms.numpy()
	lo, hi = f(nv.min()), f(nv.max())
	want_b = np.clip((((hi - nv).astype(f) / f(hi - lo)).astype(f) * f(16)).astype(np.int64), 0, 15)
	_both("norm_buckets", buckets, far, near, want_norms, want_b)
	_both("descending_norm_order", lambda M: ops.descending_norm_order(M, 16), far, near, np.argsort(want_b, kind="stable"))
	want = ivfn.renorm_rows_ref(H.float().numpy())
	ops.renorm_rows(near)
	ops.renorm_rows(far)
	torch.cuda.synchronize()
	got = far.clone()
	fl.assert_only_view_written(buf, far)
	_eq(near, want, "renorm_rows [compact]")
	_eq(got, want, "renorm_rows [far]")


# ================================================================== 2. GEMM strides
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("which,alpha", [("A", 1.0), ("B", 1.0), ("C", 1.0), ("A", 2.0), ("B", 2.0), ("C", 2.0), ("cin", 2.0)],
						 ids=["gemm-A", "gemm-B", "gemm-C", "gemm_ex-A", "gemm_ex-B", "gemm_ex-C", "gemm_ex-cin"])
def test_gemm_with_one_far_operand(ops, which, alpha, dt):
	"""alpha = 1 without cin goes through anncur_gemm, anything else through anncur_gemm_ex (ops.gemm)."""
	al = int(alpha)
	K, N = 300, 70
	A = _ints(5, K, 4, 12)
	B = _ints(K, N, 4, 13)
	Cin = _ints(5, N, 50, 14)
	if which == "A":      # a_sm
		far, near, _ = _put(A, DT[dt])
		Bd = B.to(DT[dt]).cuda()
		_both("gemm, A far", lambda M: ops.gemm(M, Bd, alpha=alpha), far, near, (al * (A @ B)).float())
	elif which == "B":    # b_sn: the transposed operand, B = Bt^T with Bt's rows far apart
		Bt = _ints(5, K, 4, 15)
		far, near, _ = _put(Bt, DT[dt])
		Ad = _ints(N, K, 4, 16).to(DT[dt]).cuda()
		_both("gemm, B far", lambda M: ops.gemm(Ad, M.t(), alpha=alpha), far, near, (al * (_ints(N, K, 4, 16) @ Bt.t())).float())
	else:
		Ad, Bd = A.to(DT[dt]).cuda(), B.to(DT[dt]).cuda()
		if which == "C":
			view, buf = _far(5, torch.float32)
			out = view[:, :N]
			ops.gemm(Ad, Bd, out=out, alpha=alpha)
			torch.cuda.synchronize()
			got = out.clone()
			fl.assert_only_view_written(buf, out)
			_eq(got, (al * (A @ B)).float(), "gemm, C far")
			_eq(ops.gemm(Ad, Bd, alpha=alpha), (al * (A @ B)).float(), "gemm, C compact")
		else:
			far, near, _ = _put(Cin, torch.float32)
			_both("gemm_ex, cin far", lambda M: ops.gemm(Ad, Bd, alpha=2.0, beta=-1.0, cin=M), far, near, (2 * (A @ B) - Cin).float())


# ================================================================== 3. the query operand of the fused family (ldx)
Q5, I_F, K_F = 5, 8203, 10
_LEAD = {"leading_sample": True, "ids": True}
# every body the plan offers at Q = 5, I = 8203, k = 10 (qt1 at Kp = 64 / 512 and staged at Kp = 512 are ignored by the plan: not listed), and
# what each flag must change in the plan against the default of its Kp: (QT, lg, ladder)
_BODIES = [(64, {}), (64, {"mfma32": True}), (64, {"staged": True}), (64, _LEAD),
		   (128, {}), (128, {"qt1": True}), (128, {"mfma32": True}), (128, {"staged": True}), (128, _LEAD),
		   (256, {}), (256, {"qt1": True}), (256, {"mfma32": True}), (256, {"staged": True}), (256, _LEAD),
		   (512, {}), (512, {"mfma32": True}), (512, _LEAD), (640, {}), (640, _LEAD)]
_PLAN_OF_FLAG = {"qt1": (1, 2, False), "mfma32": (None, 2, False), "staged": (None, 1, False)}   # None: the default's QT


@pytest.mark.parametrize("Kp,kw", _BODIES, ids=[f"Kp{b[0]}-{'-'.join(b[1]) or 'default'}" for b in _BODIES])
def test_score_topk_fused_with_far_query_rows(ops, Kp, kw):
	kw = dict(kw)
	perm = torch.randperm(I_F, generator=torch.Generator().manual_seed(Kp)) if kw.pop("ids", False) else None
	base, plan = ops.fused_plan(Q5, I_F, Kp, K_F), ops.fused_plan(Q5, I_F, Kp, K_F, **kw)
	word = lambda p: (p["QT"], p["lg"], p["ladder"])
	assert word(base) == {64: (2, 1, True), 128: (2, 1, True), 256: (2, 1, True), 512: (1, 1, False), 640: (2, 4, False)}[Kp], base
	for flag in kw:
		if flag in _PLAN_OF_FLAG:     # the flag reached the plan: another body than the default's, not a silent duplicate of it
			qt, lg, ladder = _PLAN_OF_FLAG[flag]
			assert word(plan) == (qt or base["QT"], lg, ladder) != word(base), (flag, plan)
		elif Kp <= 512:               # leading_sample: the sweep's flush period changes with it (the wide plan has no such word; its ids are checked below)
			assert word(plan) == word(base) and plan["stage_flush"] != base["stage_flush"], plan
	K = Kp - 7 if Kp <= 512 else 513
	X, E, S = fx.dense_case(Q5, I_F, K, seed=Kp)
	Xc, Etp = fx.device_operands(ops, X, E, Kp)
	view, _ = _far(5, torch.bfloat16, decoy=1.0)                            # finite everywhere: see _far
	Xf = view[:, :Kp]
	Xf.copy_(Xc)
	want_v, want_rows = fx.reference_topk(S, K_F)
	want_i = perm[want_rows] if perm is not None else want_rows
	ids = perm.int().cuda() if perm is not None else None
	nfb = {}
	for name, Xq in (("compact", Xc), ("far", Xf)):
		ws = fx.poisoned_workspace(ops, Q5, I_F, Kp, K_F)
		got, fb = ops.score_topk_fused(Xq, Etp, I_F, K_F, workspace=ws, item_ids=ids, return_fallbacks=True, **kw)
		torch.cuda.synchronize()
		nfb[name] = int(fb[0].item())
		_eq(got.values, want_v.float(), f"score_topk_fused [{name}] values")
		_eq(got.indices, want_i, f"score_topk_fused [{name}] ids")
	assert nfb["far"] == nfb["compact"], f"queries repaired by the select: {nfb}"


@pytest.mark.parametrize("Kp", [64, 128, 256, 512])
def test_score_rank_with_far_query_rows(ops, Kp):
	X, E, S = fx.dense_case(Q5, I_F, Kp - 7, seed=Kp + 1, xmax=1, emax=1)
	Xc, Etp = fx.device_operands(ops, X, E, Kp)
	view, _ = _far(5, torch.bfloat16)
	Xf = view[:, :Kp]
	Xf.copy_(Xc)
	ids = torch.randint(0, I_F, (Q5, 6), generator=torch.Generator().manual_seed(Kp), dtype=torch.int32)
	ids[:, 0], ids[:, 1] = -1, I_F - 1
	want_score = torch.where(ids < 0, torch.tensor(float("nan")), torch.gather(S, 1, ids.clamp(min=0).long()).float())
	_both("score_rank", lambda Xq: ops.score_rank(Xq, Etp, I_F, ids, return_scores=True), Xf, Xc, rank_ref(S.float().numpy(), ids.numpy()), want_score)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("which", ["X", "Et"])
def test_rescore_topk_with_far_rows(ops, which, dt):
	K, I = 70, 67
	X, E = _ints(5, K, 4, 20), _ints(I, K, 4, 21)
	S = X @ E.t()
	g = torch.Generator().manual_seed(22)
	rest = torch.tensor([i for i in range(I) if i not in (0, 33, 66)])
	cand = torch.stack([torch.cat([torch.tensor([66, 33, 0, -1]), rest[torch.randperm(I - 3, generator=g)[:36]]]) for _ in range(5)]).int()
	# (distinct item rows on every side of both lines, a hole)
	k_out = 39                                                            # every candidate but the hole comes back: a far item row read wrong shows whatever its score
	ref = [rerank_ref(S[q].numpy(), cand[q].numpy(), k_out) for q in range(5)]
	want = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
	cd = cand.cuda()
	if which == "X":
		far, near, _ = _put(X, DT[dt])
		Ed = E.to(DT[dt]).cuda()
		_both("rescore_topk, X far", lambda M: tuple(ops.rescore_topk(M, Ed, cd, k_out)), far, near, *want)
	else:
		far, near, _ = _put(E, DT[dt])
		Xd = X.to(DT[dt]).cuda()
		_both("rescore_topk, Et far", lambda M: tuple(ops.rescore_topk(Xd, M, cd, k_out)), far, near, *want)


def test_score_topk_split_with_far_query_rows(ops):
	K = 100
	X, E, S = fx.dense_case(Q5, I_F, K, seed=30)
	far, near, _ = _put(X.long(), torch.float32)
	Ed = E.cuda()
	Etp = ops.pack_split_bf16(Ed, 1, row_multiple=32)
	want_v, want_rows = fx.reference_topk(S, K_F)
	_both("score_topk_split", lambda M: tuple(ops.score_topk_split(M, Ed, Etp, I_F, K_F)), far, near, want_v.float(), want_rows)


# ================================================================== 4. id rows
def test_sort_id_rows_far_in_and_out(ops):
	w = 100
	g = torch.Generator().manual_seed(40)
	ids = torch.stack([torch.randperm(5000, generator=g)[:w] for _ in range(5)]).int()
	ids[:, ::9] = -1
	sc = _ints(5, w, 1000, 41).float()
	key = torch.where(ids < 0, torch.tensor(1 << 40), ids.long())
	order = torch.argsort(key, dim=1, stable=True)
	want_ids, want_sc, want_n = torch.gather(ids, 1, order), torch.gather(sc, 1, order), (ids >= 0).sum(1)
	view, buf = _far(5, torch.float32)
	P, start = view.stride(0), view.storage_offset()
	as_int = buf.view(torch.int32)
	fi, fs = as_int.as_strided((5, w), (P, 1), start), buf.as_strided((5, w), (P, 1), start + 1024)          # inputs: one pitch, as the kernel takes them
	oi, os_ = as_int.as_strided((5, w), (P, 1), start + 2048), buf.as_strided((5, w), (P, 1), start + 3072)  # outputs
	fi.copy_(ids.cuda())
	fs.copy_(sc.cuda())
	got = ops.sort_id_rows(fi, fs, out=(oi, os_))
	torch.cuda.synchronize()
	_eq(got[0], want_ids, "sort_id_rows ids [far]")
	_eq(got[1], want_sc, "sort_id_rows scores [far]")
	_eq(got[2], want_n, "sort_id_rows counts [far]")
	assert torch.equal(fi.cpu(), ids) and torch.equal(fs.cpu(), sc)
	fl.assert_only_view_written(buf, view)                               # (the four views lie inside the 8192-column far view)
	near = ops.sort_id_rows(ids.cuda(), sc.cuda())
	_eq(near[0], want_ids, "sort_id_rows ids [compact]")
	_eq(near[1], want_sc, "sort_id_rows scores [compact]")


def test_filter_topk_with_far_candidate_rows(ops):
	n_cand, k_out = 60, 20
	g = torch.Generator().manual_seed(42)
	idx = torch.stack([torch.randperm(5000, generator=g)[:n_cand] for _ in range(5)]).int()
	idx[:, 3::11] = -1                                                    # holes
	val = torch.sort(_ints(5, n_cand, 1000, 43).float(), dim=1, descending=True).values
	excl = [sorted(set(idx[q, 1::4].tolist()) - {-1}) + [4999 - q] for q in range(5)]
	want_v, want_i = torch.full((5, k_out), float("-inf")), torch.full((5, k_out), -1)
	for q in range(5):
		keep = [j for j in range(n_cand) if idx[q, j] >= 0 and int(idx[q, j]) not in excl[q]][:k_out]
		want_v[q, :len(keep)], want_i[q, :len(keep)] = val[q, keep], idx[q, keep].long()
	ex = ops.exclusion(excl, 5, 5000, "cuda")
	view, buf = _far(5, torch.float32)
	P, start = view.stride(0), view.storage_offset()
	fv, fi = buf.as_strided((5, n_cand), (P, 1), start), buf.view(torch.int32).as_strided((5, n_cand), (P, 1), start + 1024)   # one pitch (ld_in)
	fv.copy_(val.cuda())
	fi.copy_(idx.cuda())
	for name, (v, i) in (("compact", (val.cuda(), idx.cuda())), ("far", (fv, fi))):
		got = ops.filter_topk(v, i, ex, k_out)
		torch.cuda.synchronize()
		_eq(got.values, want_v, f"filter_topk values [{name}]")
		_eq(got.indices, want_i, f"filter_topk ids [{name}]")


@pytest.mark.parametrize("dt", BOTH)
def test_rerank_scored_with_far_score_rows(ops, dt):
	"""ld_sh (shared scores, fp32 and bf16) and ld_pq (candidate ids and scores, one pitch) far; k = the whole pool, so every entry comes back."""
	n_sh, n_pq = 24, 30
	g = torch.Generator().manual_seed(44)
	pool = torch.randperm(5000, generator=g)
	shared = torch.sort(pool[:n_sh]).values
	cand = torch.stack([pool[n_sh:][torch.randperm(4000, generator=g)[:n_pq]] for _ in range(5)]).int()
	cand[:, 2], cand[:, 4] = shared[3].int(), -1                          # a candidate that is a shared id (dropped), a hole
	sh_sc, cd_sc = _ints(5, n_sh, 100, 45), _ints(5, n_pq, 100, 46)
	k = n_sh + n_pq
	want_v, want_i = torch.full((5, k), float("-inf")), torch.full((5, k), -1)
	for q in range(5):
		score = {int(i): float(s) for i, s in zip(shared, sh_sc[q])}
		for i, s in zip(cand[q].tolist(), cd_sc[q].tolist()):
			if i >= 0 and i not in score: score[i] = float(s)
		order = sorted(score, key=lambda i: (-score[i], i))
		want_v[q, :len(order)], want_i[q, :len(order)] = torch.tensor([score[i] for i in order]), torch.tensor(order)
	view, buf = _far(5, torch.float32)
	P, start = view.stride(0), view.storage_offset()
	fc, fs = buf.view(torch.int32).as_strided((5, n_pq), (P, 1), start + 1024), buf.as_strided((5, n_pq), (P, 1), start + 2048)
	fc.copy_(cand.cuda())
	fs.copy_(cd_sc.float().cuda())
	if dt == "f32":
		far_sh, near_sh = view[:, :n_sh], sh_sc.float().cuda()
		far_sh.copy_(near_sh)
	else:
		far_sh, near_sh, _ = _put(sh_sc, torch.bfloat16)
	sid = ops.shared_id_list(shared.tolist(), "cuda")
	for name, (c, s, sh) in (("compact", (cand.cuda(), cd_sc.float().cuda(), near_sh)), ("far", (fc, fs, far_sh))):
		got = ops.rerank_scored(k, cand=c, cand_scores=s, shared_ids=sid, shared_scores=sh)
		torch.cuda.synchronize()
		_eq(got.values, want_v, f"rerank_scored values [{name}]")
		_eq(got.indices, want_i, f"rerank_scored ids [{name}]")


def _lstsq_seed():
	"""The first seed whose hadamard_case names item rows below 2^31, in [2^31, 2^32) and the one beyond 2^32 (row 66 of 67)."""
	for seed in range(1000):
		item_of = np.random.default_rng(seed).permutation(67)[:20]           # hadamard_case's first draw
		if 66 in item_of and (item_of < 33).any() and ((item_of >= 33) & (item_of < 66)).any():
			return seed


@pytest.mark.parametrize("which", ["Rt", "ids_C", "W"])
def test_lstsq_rows_with_far_operands(ops, which):
	"""Signed Hadamard columns (tests/test_gpu_lstsq_rows.py hadamard_case): W = S / 64 is an fp32 number, bit for bit.  Rt [67 x 64] with far
	rows (every query's 20 ids spread over all three offset ranges), or ids and C [5 x 22] at a far pitch."""
	import test_gpu_lstsq_rows as lr
	Rt, ids, C, S = lr.hadamard_case(64, list(range(3, 63, 3)), 5, _lstsq_seed(), hole_pos=(0, 8))
	named = ids[ids >= 0].unique().cpu()
	assert tuple(Rt.shape) == (67, 64) and 66 in named and (named < 33).any() and ((named >= 33) & (named < 66)).any()
	want = lr.exact_f32(S, 64)
	if which == "Rt":
		view, _ = _far(67, torch.float32)
		Rf = view[:, :64]
		Rf.copy_(Rt)                                                      # (the rows no id names stay NaN, as in the compact twin)
		cases = (("compact", Rt, ids, C), ("far", Rf, ids, C))
	elif which == "W":   # the output (ldw) far: alone in its allocation, which must be poison everywhere else afterwards
		view, buf = _far(5, torch.float32)
		Wf = view[:, :64]
		st = torch.full((5,), -1, dtype=torch.int32, device="cuda")
		ops.lstsq_rows(Rt, ids, C, out=(Wf, st))
		torch.cuda.synchronize()
		got = Wf.clone()
		fl.assert_only_view_written(buf, Wf)
		assert not st.cpu().any()
		_eq(got, want, "lstsq_rows, W far")
		return
	else:
		n = ids.shape[1]
		view, buf = _far(5, torch.float32)
		P, start = view.stride(0), view.storage_offset()
		Cf, If = buf.as_strided((5, n), (P, 1), start), buf.view(torch.int32).as_strided((5, n), (P, 1), start + 1024)
		Cf.copy_(C)
		If.copy_(ids)
		cases = (("compact", Rt, ids, C), ("far", Rt, If, Cf))
	for name, R, i, c in cases:
		W = torch.full((5, 64), float("nan"), device="cuda")
		st = torch.full((5,), -1, dtype=torch.int32, device="cuda")
		ops.lstsq_rows(R, i, c, out=(W, st))
		torch.cuda.synchronize()
		assert not st.cpu().any(), (name, st)
		_eq(W, want, f"lstsq_rows W [{name}]")


def test_lstsq_state_seed_and_extend_with_far_item_rows(ops):
	"""LstsqState.seed_shared + two extend calls on the same Hadamard data with ONE id order for all queries (the first 6 positions are the
	shared prefix), Rt's rows far: after each extend W is the exact rational result of the positions absorbed so far."""
	import test_gpu_lstsq_rows as lr
	Rt, ids, C, _ = lr.hadamard_case(64, list(range(3, 63, 3)), 5, _lstsq_seed(), hole_pos=(10, 15))
	ids = ids[:1].expand(5, -1).contiguous()
	row0 = ids[0].cpu()
	assert 66 in row0 and (row0[:6] >= 0).all()
	R = torch.nan_to_num(Rt.cpu()).double()                               # (only named rows are read)

	def want(n):
		keep = row0[:n] >= 0
		return lr.exact_f32((C[:, :n].cpu().double()[:, keep] @ R[row0[:n][keep].long()]).numpy(), 64)
	view, _ = _far(67, torch.float32)
	Rf = view[:, :64]
	Rf.copy_(Rt)
	for name in ("compact", "far", "W far"):
		wbuf = None
		if name == "W far":   # the output (ldw) in a far view of its own, Rt compact (one fp32 far buffer at a time: this evicts Rt's)
			Rf = view = state = None
			wview, wbuf = _far(5, torch.float32)
			Wf = wview[:, :64]
		state = ops.LstsqState(Rf if name == "far" else Rt, 5, cap=ids.shape[1])
		state.seed_shared(row0[:6].tolist())
		for n in (12, ids.shape[1]):
			out = None if wbuf is None else (Wf, torch.full((5,), -1, dtype=torch.int32, device="cuda"))
			W, st = state.extend(ids[:, :n], C[:, :n], out=out)
			torch.cuda.synchronize()
			assert not st.cpu().any(), (name, n, st)
			_eq(W.clone(), want(n), f"LstsqState.extend to {n} positions [{name}]")
			if wbuf is not None:
				fl.assert_only_view_written(wbuf, Wf)


# ================================================================== 5. anchor block
@pytest.mark.parametrize("dt", BOTH)
def test_select_pivoted_with_far_rows(ops, dt):
	m, k = 3001, 64
	g = np.random.default_rng(50)
	scales = g.integers(-256, 257, m)
	R = torch.from_numpy(pn.hadamard_items(scales, kq=67))
	far, near, _ = _put(R, DT[dt])
	want_ids, want_gains, n_sel = pn.hadamard_closed_form(scales, k)
	for name, M in (("compact", near), ("far", far)):
		ids, gains, n = ops.select_pivoted(M, k)
		assert n == n_sel, (name, n, n_sel)
		_eq(ids, want_ids, f"select_pivoted ids [{name}]")
		_eq(gains, want_gains, f"select_pivoted gains [{name}]")


@pytest.mark.parametrize("shape", [(5, 3), (3, 5)])
def test_svd_jacobi_on_a_far_block(ops, shape):
	rows, cols = shape
	H = _ints(5, 8, 9, 60)
	far, near, _ = _put(H, torch.float32)
	Wf, Wn = (far[:, :3], near[:, :3]) if rows == 5 else (far[::2, :5], near[::2, :5])   # (3 rows: 0, 2 and 4 -- the pitch doubles, the last row stays beyond 2^32)
	assert Wf.stride(0) * (rows - 1) >= 1 << 32
	a, b = ops.svd_jacobi(Wn), ops.svd_jacobi(Wf)
	torch.cuda.synchronize()
	assert a.converged and b.converged and a.sweeps == b.sweeps
	for x, y in ((a.U, b.U), (a.S, b.S), (a.V, b.V)):
		assert torch.equal(x.view(torch.int64), y.view(torch.int64))
	assert torch.isfinite(b.S).all()                                     # (the compact call's values are checked in tests/test_gpu_svd.py; the poison is NaN)


# ================================================================== 6. IVF (Xs far)
IVF_SIZES = np.array([700, 0, 900, 1390, 10], dtype=np.int64)             # list 2 straddles row 1500 (2^31 elements), list 4 row 2999 (2^32); list 1 is empty


def _ivf_data(dp, seed, nq=5):
	g = np.random.default_rng(seed)
	n = int(IVF_SIZES.sum())
	off = np.concatenate([[0], np.cumsum(IVF_SIZES)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X = g.integers(-8, 9, (n, dp)).astype(np.int64)
	Qh = g.integers(-8, 9, (nq, dp)).astype(np.int64)
	# The far vectors must WIN: a vector row read from the poison scores NaN and silently leaves a top-k it was not part of anyway.  Every
	# query carries 8 in its first 32 columns; the ten vectors of list 4 (rows 2990..2999, the last beyond 2^32 elements) carry 8 there too
	# (+2048), five rows beyond 2^31 of each of the lists 2 and 3 carry 8 in the first 24 (+1536), every other vector is <= 0 there (-1075 on
	# average): ten standard deviations of the other columns' contribution (<= 24 sqrt(96) = 235) apart.  With k = IVF_K = 20 every planted vector of a list the query probes is in its result (every query probes
	# at least one of the three lists).
	X[:, :32] = -np.abs(X[:, :32])
	Qh[:, :32] = 8
	X[2990:3000, :32] = 8
	for r0 in (1550, 2000):
		X[r0:r0 + 5, :24] = 8
	probe = np.array([[2, 4, 0], [4, 3, 1], [1, 2, 3], [3, 4, 2], [0, 1, 4]], dtype=np.int32)
	return off, ids, X, Qh, probe


IVF_K = 20


def _ivf_planted_found(want_ids, ids, probe):
	"""The reference itself names the planted vectors of every probed list (so the data do what the comment above says)."""
	for q in range(probe.shape[0]):
		rows = [r for lst, r0, n in ((4, 2990, 10), (2, 1550, 5), (3, 2000, 5)) if lst in probe[q] for r in range(r0, r0 + n)]
		assert rows
		assert set(int(ids[r]) for r in rows) <= set(int(i) for i in want_ids[q]), q


@pytest.mark.parametrize("dp", [80, 128])
def test_ivf_list_means_and_scan_with_far_vectors(ops, dp):
	off, ids, X, Qh, probe = _ivf_data(dp, 70 + dp)
	far, near, _ = _put(torch.from_numpy(X), torch.float32)
	assert far.stride(0) * 1499 < 1 << 31 <= far.stride(0) * 1500 and far.stride(0) * 2999 >= 1 << 32
	off_d, ids_d = torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda()
	C0 = np.full((5, dp), 7.0, dtype=np.float32)
	want = ivfn.list_means_ref(X[:, :dp], off, C0)
	_both("ivf_list_means", lambda M: ops.ivf_list_means(M, off_d, torch.from_numpy(C0.copy()).cuda()), far, near, want)
	Qd, pd = torch.from_numpy(Qh).float().cuda(), torch.from_numpy(probe).cuda()
	w = ivfn.lists_search_ref(X, Qh, off, ids, probe, IVF_K, ("id",))["id"]
	_ivf_planted_found(w[1], ids, probe)
	_both("ivf_scan", lambda M: tuple(ops.ivf_scan(M, off_d, ids_d, Qd, pd, IVF_K)), far, near, w[0], w[1])


@pytest.mark.parametrize("q_far", [False, True], ids=["Qcompact", "Qfar"])
@pytest.mark.parametrize("dt,dp", [("f32", 80), ("bf16", 80), ("bf16", 128)])
def test_ivf_search_grouped_with_far_vectors(ops, dt, dp, q_far):
	off, ids, X, Qh, probe = _ivf_data(dp, 71 + dp)
	far, near, _ = _put(torch.from_numpy(X), DT[dt])
	off_d, ids_d, pd = torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(probe).cuda()
	Qd = torch.from_numpy(Qh).to(DT[dt]).cuda()
	if q_far and dt == "bf16":   # a second 16-bit far buffer, in the fp32 slot (12 + 12 GiB)
		qv, _ = _far(5, torch.bfloat16, slot="f32")
		Qf = qv[:, :dp]
	elif q_far:                  # beside 24 GiB of fp32 vectors: the 16-bit slot's 12 GiB seen as fp32 -- half the pitch, row 4 at element 2^31 + 16, byte 2^33 + 64
		qv, qbuf = _far(5, torch.bfloat16)
		Qf = qbuf.view(torch.float32).as_strided((5, dp), (qv.stride(0) // 2, 1), qv.storage_offset() // 2)
		assert Qf.stride(0) * 4 >= 1 << 31
	if q_far:
		Qf.copy_(Qd)
		Qd = Qf
	want = ivfn.lists_search_ref(X, Qh, off, ids, probe, IVF_K, ("packed",))["packed"]
	_ivf_planted_found(want[1], ids, probe)

	def call(M):
		for cls, v in ((ops._ScoreScratch, float("inf")), (ops._ByteScratch, 0xff)):
			for b in cls._bufs.values(): b.fill_(v)
		return tuple(ops.ivf_search_grouped(M, off_d, ids_d, IVF_SIZES, Qd, pd, IVF_K))
	_both("ivf_search_grouped", call, far, near, want[0], want[1])


# ================================================================== 7. an item matrix beyond 2^31 elements
BIG = [(512, (1 << 31) // 512 + 101), (640, (1 << 31) // 640 + 101), (256, (1 << 31) // 256 + 101)]
QB, KB = 32, 10


def _big_case(Kp, I):
	"""Etp [ceil32(I) x Kp] bf16 built on the device, bulk entries integers in [-100, 100].  Query q is e_q + 2^-8 e_(32 + q): its bulk scores
	E[i, q] + E[i, 32 + q] / 256 are exact, below 101 in magnitude and spread over 201^2 levels (few ties at the threshold).  KB planted items,
	shared by the queries: in the first tile (its first and last row), on both sides of element 2^31 (the row that ends at or straddles it and
	the next), 40 rows on, in the last full tile (first and last row), in the tail (last two rows), and one bulk position.  Item j scores
	200 - 2 ((j + q) mod KB) for query q: every query has its own order.  -> (Xp, Etp, planted rows [KB], rank of item j for query q [QB x KB])."""
	Ip = -(-I // 32) * 32
	line = (1 << 31) // Kp                                                  # the row that holds element 2^31
	assert line * Kp <= 1 << 31 < I * Kp and I - line == 101 and I % 32 >= 2
	last_full = (I // 32 - 1) * 32
	plant = torch.tensor([0, 31, line - 1, line, line + 40, last_full, last_full + 31, I - 2, I - 1, 1000])
	assert plant.unique().numel() == KB and line + 40 < last_full and last_full + 31 < I - 2
	torch.manual_seed(Kp)
	E = torch.empty((Ip, Kp), dtype=torch.bfloat16, device="cuda")
	for r0 in range(0, Ip, 1 << 20):
		r1 = min(Ip, r0 + (1 << 20))
		E[r0:r1] = torch.randint(-100, 101, (r1 - r0, Kp), device="cuda", dtype=torch.int8).to(torch.bfloat16)
	E[I:] = 0
	order = (torch.arange(KB)[None, :] + torch.arange(QB)[:, None]) % KB       # [q, j]
	E[plant.cuda(), :QB] = (200 - 2 * order.t()).to(torch.bfloat16).cuda()
	E[plant.cuda(), 32:32 + QB] = 0
	X = torch.zeros((QB, Kp), dtype=torch.bfloat16, device="cuda")
	X[torch.arange(QB), torch.arange(QB)] = 1
	X[torch.arange(QB), 32 + torch.arange(QB)] = 2.0 ** -8
	return X, E, plant, order


@pytest.mark.parametrize("Kp,I", BIG, ids=[f"Kp{b[0]}" for b in BIG])
def test_item_matrix_beyond_2_31_elements(ops, Kp, I):
	_SLOT.clear()
	torch.cuda.empty_cache()
	assert ops.fused_supported(QB, I, Kp, KB), "the plan refuses the shape"
	X, E, plant, order = _big_case(Kp, I)
	want_v = (200 - 2 * torch.arange(KB)).float().expand(QB, KB)
	want_i = plant[torch.argsort(order, dim=1)]                             # query q's t-th item: the j with (j + q) mod KB = t
	got = ops.score_topk_fused(X, E, I, KB, workspace=fx.poisoned_workspace(ops, QB, I, Kp, KB))
	_eq(got.values, want_v, "default body: values")
	_eq(got.indices, want_i, "default body: items")
	perm = torch.randperm(I, device="cuda").int()
	got = ops.score_topk_fused(X, E, I, KB, workspace=fx.poisoned_workspace(ops, QB, I, Kp, KB), leading_sample=True, item_ids=perm)
	_eq(got.values, want_v, "leading_sample + item_ids: values")
	_eq(got.indices, perm.cpu().long()[want_i], "leading_sample + item_ids: items")
	if Kp <= 512:
		rank, score = ops.score_rank(X, E, I, plant.int().expand(QB, KB).contiguous(), return_scores=True)
		_eq(rank, order, "score_rank of the planted items")
		_eq(score, (200 - 2 * order).float(), "score_rank scores")
	cand = torch.cat([plant.flip(0), torch.tensor([-1, 77])]).int().expand(QB, KB + 2).contiguous().cuda()   # the planted items, a hole, one bulk item
	got = ops.rescore_topk(X, E[:I], cand, KB)
	_eq(got.values, want_v, "rescore_topk values")
	_eq(got.indices, want_i, "rescore_topk items")
	del X, E
	torch.cuda.empty_cache()
