"""Subnormal operands, products and sums through the order-sensitive routes: anncur_gemm / anncur_gemm_ex (csrc/gemm.hip, the fp32 MFMA and
its epilogue), anncur_rescore_topk (csrc/split.hip, "the chain anncur_gemm is, bit for bit") and the split-bf16 route.  The other
families are in tests/test_gpu_subnormal_fused.py (fused top-k, small batch, the error sums) and tests/test_gpu_subnormal_routes.py
(ranks, selectors, IVF, sparse, the fp64 gather).

Every expected value is a host reference of tests/subnormal_cases.py (held on the host by tests/test_cpu_subnormal_reference.py): the
IEEE form.  Its DAZ and FTZ forms say what a flush would give; each case asserts on the host, before it launches, that the form it is
about lies far from the IEEE one (subnormal_cases.assert_chain_case).  Nothing is read back from the device to form an expectation, no
comparison has a tolerance, everything goes through integer views.  Operands are views into NaN-filled buffers and outputs views into
buffers pre-filled with a NaN pattern no kernel produces (the helpers of tests/test_gpu_gemm_exact.py).

What the build promises is held by tests/test_cpu_denorm_mode.py (float_denorm_mode 3 / 3 in every kernel descriptor).
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subnormal_cases as sn  # noqa: E402
import test_gpu_gemm_exact as ge  # noqa: E402  (its poisoned-buffer helpers; pytest collects none of its tests from here)
from oracle import gemm_chain as G  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
_DTYPE_IDS = lambda v: "".join("hf"[not x] for x in v)  # noqa: E731


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _want(acc, out_dtype):
	"""fp32 reference -> host tensor of the output type; bf16: one more round-to-nearest-even, into bf16's subnormals where the value is one."""
	if out_dtype == F32:
		return torch.from_numpy(np.ascontiguousarray(acc))
	return torch.from_numpy(sn.f32_to_bf16_rne(acc).view(np.int16)).view(BF16)


def _which(got_bits, refs):
	"""For a failure message: which of the three references the device's bits equal, if any."""
	return [name for name, r in refs.items() if np.array_equal(got_bits, sn.bits32(r))] or "none of ieee / daz / ftz"


# ------------------------------------------------------------------ 1. anncur_gemm: the chain with subnormal sums and subnormal operands
@pytest.mark.parametrize("dtypes", G.DTYPES, ids=_DTYPE_IDS)
@pytest.mark.parametrize("layout", sn.CHAIN_LAYOUTS, ids="".join)
@pytest.mark.parametrize("M,N,K", sn.CHAIN_SHAPES)
@pytest.mark.parametrize("case", list(sn.CHAIN_CASES))
def test_gemm_equals_the_ieee_chain(ops, case, M, N, K, layout, dtypes):
	A, B, sa, sb = sn.chain_operands(case, M, N, K, dtypes[0], dtypes[1], seed=1)
	refs = sn.chain_references(A, B, sa, sb)
	sn.assert_chain_case(case, A, B, refs)
	acc = refs["ieee"]
	a, b = ge._place(A, layout[0], ge._dt(dtypes[0])), ge._place(B, layout[1], ge._dt(dtypes[1]))
	got = sn.bits32(ops.gemm(a, b).cpu().numpy())
	assert np.array_equal(got, sn.bits32(acc)), f"{case}: {(got != sn.bits32(acc)).mean():.2f} of the elements differ from the IEEE chain; the device equals {_which(got, refs)}"
	for out_dtype, kind in ((F32, "p"), (F32, "pt"), (BF16, "s2"), (BF16, "p")):
		buf, out = ge._poisoned_out(kind, M, N, out_dtype)
		assert ops.gemm(a, b, out=out) is out
		ge._assert_buffer(buf, kind, _want(acc, out_dtype), out_dtype, f"{case} out {kind} {out_dtype}")
	if case == "sums":   # the bf16 output of a subnormal fp32 is a bf16 subnormal (or rounds to zero, or up to 2^-126): the case has them
		w16 = sn.f32_to_bf16_rne(acc)
		assert sn.is_subnormal_bits16(w16).mean() >= 0.1


@pytest.mark.parametrize("cin_kind", ["separate", "strided", "is_out"])
@pytest.mark.parametrize("beta", [2.0, -0.25])
@pytest.mark.parametrize("alpha", [2.0, -0.25])
def test_gemm_ex_epilogue_on_a_subnormal_accumulator_and_subnormal_cin(ops, alpha, beta, cin_kind):
	"""out = alpha acc + beta Cin with acc = n 2^-147 and Cin = c 2^-147: order-free data on which both scalings are exact even by 1/4
	(subnormal_cases.epilogue_operands), so the expected bits hold for a contracted and for an uncontracted epilogue alike.  A flushed
	accumulator, Cin or result shows as zeros: more than 90 % of the expected values are subnormal."""
	M, N, K = 65, 129, 33
	A, B, Cin, acc = sn.epilogue_operands(M, N, K, seed=3)
	want = sn.epilogue_reference(acc, alpha, beta, Cin)
	assert sn.is_subnormal(want).mean() > 0.9
	a, b = ge._place(A, "p", F32), ge._place(B, "t", BF16)
	if cin_kind == "is_out":
		for kind in ge.OUT_KINDS:
			buf, out = ge._poisoned_out(kind, M, N, F32)
			out.copy_(torch.from_numpy(Cin))
			ge._assert_buffer(buf, kind, torch.from_numpy(Cin), F32, "test setup")
			ops.gemm(a, b, out=out, alpha=alpha, beta=beta, cin=out)
			ge._assert_buffer(buf, kind, _want(want, F32), F32, f"cin is out, {kind}")
		return
	cin = ge._place(Cin, "n" if cin_kind == "separate" else "g", F32)
	cin_bits = cin.clone()
	for out_dtype in (F32, BF16):
		for kind in ge.OUT_KINDS:
			buf, out = ge._poisoned_out(kind, M, N, out_dtype)
			ops.gemm(a, b, out=out, alpha=alpha, beta=beta, cin=cin)
			ge._assert_buffer(buf, kind, _want(want, out_dtype), out_dtype, f"cin {cin_kind}, out {kind} {out_dtype}")
	assert torch.equal(cin.view(torch.int32), cin_bits.view(torch.int32))
	got = ops.gemm(a, b, alpha=alpha).cpu().numpy()      # alpha alone: no Cin term at all, so -0.25 times an accumulator of +0 stays -0
	sn.epilogue_reference(acc, alpha, 0.0, np.zeros_like(Cin))
	assert np.array_equal(sn.bits32(got), sn.bits32(G.epilogue(acc, alpha)))


@pytest.mark.parametrize("beta", [2.0, -0.25])
def test_gemm_ex_epilogue_on_the_chain_with_subnormal_sums(ops, beta):
	"""The epilogue behind the order-sensitive `sums` chain: alpha = 2 (exact on every subnormal) and Cin = c 2^-147 (beta Cin exact)."""
	M, N, K = 33, 65, 100
	A, B, sa, sb = sn.chain_operands("sums", M, N, K, False, True, seed=2)
	refs = sn.chain_references(A, B, sa, sb)
	sn.assert_chain_case("sums", A, B, refs)
	Cin = (np.random.default_rng(9).integers(-4000, 4001, (M, N)) * 2.0 ** -147).astype(np.float32)
	G.assert_exact_in_fp64(A, B, Cin, sa=sa, sb=sb)
	want = sn.epilogue_reference(refs["ieee"], 2.0, beta, Cin)
	assert sn.is_subnormal(want).mean() >= 0.1 and sn.share(want, sn.epilogue_reference(refs["ftz"], 2.0, beta, Cin)) >= sn.MIN_FLUSH_SHARE
	a, b, cin = ge._place(A, "n", F32), ge._place(B, "p", BF16), ge._place(Cin, "g", F32)
	for out_dtype, kind in ((F32, "p"), (BF16, "s2")):
		buf, out = ge._poisoned_out(kind, M, N, out_dtype)
		ops.gemm(a, b, out=out, alpha=2.0, beta=beta, cin=cin)
		ge._assert_buffer(buf, kind, _want(want, out_dtype), out_dtype, f"beta {beta}, out {kind} {out_dtype}")


# ------------------------------------------------------------------ 2. anncur_rescore_topk and the split-bf16 route
def _by_score_then_id(scores, ids, k):
	"""Per row the k best (score, id) pairs, score descending (by value: -0 and +0 tie), ties by the smaller id.  float32 / int64 numpy."""
	order = np.lexsort((ids, -scores.astype(np.float64)), axis=-1)[:, :k]
	return np.take_along_axis(scores, order, 1), np.take_along_axis(ids, order, 1)


@pytest.mark.parametrize("dtypes", [(False, False), (True, True)], ids=_DTYPE_IDS)
@pytest.mark.parametrize("case", list(sn.CHAIN_CASES))
def test_rescore_values_bit_equal_to_the_ieee_chain(ops, case, dtypes):
	"""X [33 x 100], Et [65 x 100] (row pitch 104, NaN behind the rows), every query re-scores 40 of the 65 items in its own order: the
	values are the chain's, bit for bit, in the `sums` case subnormal for a good part and ordered among themselves."""
	Q, I, K, n_cand = 33, 65, 100, 40
	A, B, sa, sb = sn.chain_operands(case, Q, I, K, dtypes[0], dtypes[1], seed=4)
	refs = sn.chain_references(A, B, sa, sb)
	sn.assert_chain_case(case, A, B, refs)
	S = refs["ieee"]
	dt = ge._dt(dtypes[0])
	X = ge._place(A, "p", dt)
	Et = torch.full((I, K + 4), float("nan"), dtype=dt, device="cuda")[:, :K]
	Et.copy_(torch.from_numpy(np.ascontiguousarray(B.T)).to(dt))
	rng = np.random.default_rng(5)
	cand = np.stack([rng.permutation(I)[:n_cand] for _ in range(Q)]).astype(np.int64)
	sc = np.take_along_axis(S, cand, 1)
	for k_out in (1, 20, n_cand):
		want_v, want_i = _by_score_then_id(sc, cand, k_out)
		got = ops.rescore_topk(X, Et, torch.from_numpy(cand).int().cuda(), k_out)
		gv = sn.bits32(got.values.cpu().numpy())
		if not np.array_equal(gv, sn.bits32(want_v)):
			alt = {n: _by_score_then_id(np.take_along_axis(r, cand, 1), cand, k_out)[0] for n, r in refs.items()}
			raise AssertionError(f"{case} k_out={k_out}: values differ from the IEEE chain; the device equals {_which(gv, alt)}")
		assert np.array_equal(got.indices.cpu().numpy(), want_i)
	if case == "sums":
		assert sn.is_subnormal(sc).mean() >= 0.1
	# the parity claim on the same data: rescore = the element of ops.gemm(X, Et^T)
	dense = ops.gemm(X, Et.t()).cpu().numpy()
	assert np.array_equal(sn.bits32(dense), sn.bits32(S))


def _fp32_operands(case):
	X = torch.from_numpy(case.X.astype(np.float32)).cuda()
	Et = torch.from_numpy(np.ascontiguousarray(case.E.T.astype(np.float32))).cuda()
	return X, Et


@pytest.mark.parametrize("name", ["all-sub", "sub-in"])
def test_split_route_equals_the_fp32_reference(ops, name):
	"""ops.score_topk_split on fp32 operands that are bf16-exact (hi = x, lo = 0): the sweep ranks n 2^u on the bf16 MFMA, the rescore forms the
	fp32 chain.  all-sub: every score a subnormal or a zero; sub-in: every non-zero query entry a subnormal (m 2^-133), every score normal --
	and 0 for a route that reads subnormal operands as zero.  Values and ids against THE top-k of the host scores; the dense fp32 route on
	the same operands must return the same (the header's parity claim), and is held to the same reference."""
	Q, I, K, k = 70, 8209, 56, 100
	case = sn.IntCase(name, Q, I, K, k, seed=6)
	want_v, want_i = case.topk()
	assert (case.S_daz != case.S).mean() > 0.8 if name == "sub-in" else not case.S_ftz.any()
	X, Et = _fp32_operands(case)
	Etp = ops.pack_split_bf16(Et, 1, row_multiple=32)
	for route, got in (("dense", ops.score_topk_dense(X, Et, k)), ("split", ops.score_topk_split(X, Et, Etp, I, k))):
		torch.cuda.synchronize()
		gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy().astype(np.int64)
		assert np.array_equal(sn.bits32(gv), sn.bits32(want_v)), f"{route} {name}: {(sn.bits32(gv) != sn.bits32(want_v)).mean():.2f} of the values differ (all zero: {not gv.any()})"
		assert np.array_equal(gi, want_i), f"{route} {name}: ids differ in {int((gi != want_i).any(1).sum())} queries"
