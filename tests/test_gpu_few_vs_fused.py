"""The small-batch route against the fused top-k on Gaussian bf16 operands.

Kp <= 256: few_score_kernel accumulates a score over ascending k-steps of v_mfma_f32_16x16x32_bf16 into one accumulator from zero, the k order
of score16_kernel, so ops.score_topk_few's values must equal ops.score_topk_fused's on the same item-order operand BIT FOR BIT, and the ids
wherever a value is unique in its row's result (the fused route orders exact ties by row too, but only up to the body's own tie handling).
Kp >= 512: the other bodies sum in another order, so the scores of ops.score_rows_few are held to the bound of DESIGN 4.4a for a sum of Kp
exact products in fp32, |S - S_fp64| <= Kp 2^-23 (|X| . |E|^T), elementwise, against a float64 host product of the bf16 values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
I, K_TOP = 60000, 100


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _gauss(Q, Kp, seed):
	g = torch.Generator().manual_seed(seed)
	X = torch.randn(Q, Kp, generator=g).bfloat16()
	E = torch.randn(I, Kp, generator=g).bfloat16()
	return X, E


@pytest.mark.parametrize("Kp", [64, 128, 256])
@pytest.mark.parametrize("Q", [5, 64])
def test_values_bit_equal_to_the_fused_route(ops, Q, Kp):
	X, E = _gauss(Q, Kp, 100 * Q + Kp)
	Xp, Etp = ops.pack_bf16(X.cuda(), Kp), ops.pack_bf16(E.cuda(), Kp, row_multiple=32)
	assert ops.fused_supported(Q, I, Kp, K_TOP) and ops.score_topk_few_ok(Q, I, Kp, K_TOP)
	few, st = ops.score_topk_few(Xp, Etp, I, K_TOP, workspace=ops.few_workspace(Q, I, Kp, K_TOP, torch.device("cuda")), return_stats=True)
	fused = ops.score_topk_fused(Xp, Etp, I, K_TOP)
	torch.cuda.synchronize()
	fv, uv = few.values.cpu(), fused.values.cpu()
	assert torch.equal(fv.view(torch.int32), uv.view(torch.int32)), f"{(fv != uv).sum().item()} values differ"
	unique = torch.ones_like(fv, dtype=torch.bool)
	unique[:, 1:] &= fv[:, 1:] != fv[:, :-1]
	unique[:, :-1] &= fv[:, :-1] != fv[:, 1:]
	assert unique.float().mean() > 0.5
	assert torch.equal(few.indices.cpu()[unique], fused.indices.cpu()[unique])
	assert not st.fallback.any() and (st.n_cand >= K_TOP).all() and (st.groups_read >= K_TOP).all()
	# and it is the top-k of its own score rows
	S, _ = ops.score_rows_few(Xp, Etp, I)
	tv, ti = torch.topk(S, K_TOP, dim=1)
	assert torch.equal(tv.cpu().view(torch.int32), fv.view(torch.int32))


@pytest.mark.parametrize("Q,Kp", [(5, 512), (64, 512), (5, 1024)])
def test_scores_within_the_fp32_sum_bound_at_wide_kp(ops, Q, Kp):
	X, E = _gauss(Q, Kp, Q + Kp)
	Xp, Etp = ops.pack_bf16(X.cuda(), Kp), ops.pack_bf16(E.cuda(), Kp, row_multiple=32)
	S, _ = ops.score_rows_few(Xp, Etp, I)
	torch.cuda.synchronize()
	X64, E64 = X.double(), E.double()
	ref = X64 @ E64.t()
	bound = Kp * 2.0 ** -23 * (X64.abs() @ E64.abs().t())
	err = (S.cpu().double() - ref).abs()
	worst = (err / bound).max().item()
	print(f"Q={Q} Kp={Kp}: max |S - S_fp64| / bound = {worst:.3e}")
	assert (err <= bound).all(), worst
	few = ops.score_topk_few(Xp, Etp, I, K_TOP)
	tv, _ = torch.topk(S, K_TOP, dim=1)
	assert torch.equal(few.values.view(torch.int32), tv.view(torch.int32))
