"""pinv._spectral_norm_sq, info["cond_2"] and the gate of pinv_backend="auto" (cur._pinv) on the spectrum families of tests/pinv_numpy.py:
power-law, geometric, flat with one small value, and two clusters with sigma_2 / sigma_1 = 0.8 .. 0.96, each at 400 x 160, 512 x 256,
256 x 512 and 2048 x 1024, cond_2 = 300 / 700 / 1050, three seeds -- 252 blocks, 21 per test case.

The conditions come from the project's own constants, none is measured: the estimates are Rayleigh quotients, so lower bounds (1e-9 for
rounding); "auto" multiplies cond_2 by cur.AUTO_COND_SAFETY, so the estimate may be that factor short and no more; one estimate of
sigma_max^2 may then be short by its square.  The true values are numpy.linalg.svd's, in fp64, of the same fp32 block.  From these alone a
block with cond_2 = 700 stays on the device (estimate <= 700 <= 800) and one with 1050 goes to the host (estimate >= 840 > 800): no input
sits near the threshold.  tests/test_cpu_pinv_reference.py shows that the 8-step estimator this replaced failed them.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinv_numpy as P  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = [(shape, seed) for shape in P.SHAPES for seed in P.SEEDS]
GROUP_IDS = [f"{s[0]}x{s[1]}-seed{seed}" for s, seed in GROUPS]
_SINGULAR_VALUES = {}      # member -> numpy's fp64 singular values of the fp32 block: computed once, shared by both tests


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _member(member):
	"""-> (W fp32 on the host, its singular values); the block is rebuilt (a GEMM), the decomposition kept."""
	if member in _SINGULAR_VALUES:
		U, V = P.orthogonal_factors(*member[1], member[3])
		W = ((U * P.spectrum(member[0], min(member[1]), member[2])) @ V.T).astype(np.float32)
		return W, _SINGULAR_VALUES[member]
	W, S = P.build_member(member)
	S.setflags(write=False)
	_SINGULAR_VALUES[member] = S
	return W, S


@pytest.mark.parametrize("shape,seed", GROUPS, ids=GROUP_IDS)
def test_estimates_are_lower_bounds_within_the_safety_factor(ops, shape, seed):
	from anncur_amd import cur, pinv
	worst = {}
	for member in P.members(shapes=(shape,), seeds=(seed,)):
		W, S = _member(member)
		cond_true = S[0] / S[-1]
		assert abs(cond_true / member[2] - 1.0) < 0.02
		Wg = torch.from_numpy(W).cuda()
		X, info = pinv.pinv_newton_schulz_f64(Wg, return_info=True)
		s2 = pinv._spectral_norm_sq(Wg.double())
		ok = P.soundness(cond_true, S[0] ** 2, s2, info["cond_2"], cur.AUTO_COND_SAFETY)
		assert info["converged"] and all(ok.values()), (P.member_id(member), ok, info, cond_true, S[0] ** 2 / s2)
		w = worst.setdefault(member[0], [0.0, 0.0])
		w[0], w[1] = max(w[0], cond_true / info["cond_2"]), max(w[1], S[0] ** 2 / s2)
	print(f"{shape[0]} x {shape[1]} seed {seed}, {2 ** pinv.POWER_SQUARINGS} steps, worst true / cond_2 (sigma_max^2 / s2): "
		  + ", ".join(f"{f} {a:.4f} ({b:.4f})" for f, (a, b) in worst.items()))


@pytest.mark.parametrize("shape,seed", GROUPS, ids=GROUP_IDS)
def test_auto_keeps_cond_700_on_the_device_and_sends_cond_1050_to_the_host(ops, shape, seed, monkeypatch):
	from anncur_amd import cur
	host_calls = []
	real_host = cur._pinv_host

	def recording_host(M, rcond=None):
		out = real_host(M, rcond)
		host_calls.append((M.detach().cpu().clone(), rcond, out))
		return out
	monkeypatch.setattr(cur, "_pinv_host", recording_host)
	dev = torch.device("cuda")
	for member in P.members(shapes=(shape,), seeds=(seed,), conds=(700.0, 1050.0)):
		W, S = _member(member)
		Wt = torch.from_numpy(W)
		del host_calls[:]
		U = cur._pinv(Wt, dev, "auto")
		assert U.dtype == torch.float32 and tuple(U.shape) == (shape[1], shape[0]) and U.is_cuda
		if member[2] == 1050.0:
			# the host route: exactly one call of cur._pinv_host, on this block, with the reference's rcond, and its result bit for bit
			assert len(host_calls) == 1, P.member_id(member)
			M, rcond, out = host_calls[0]
			assert rcond is None and torch.equal(M, Wt)
			assert torch.equal(U.cpu().view(torch.int32), out.view(torch.int32)), P.member_id(member)
			continue
		assert not host_calls, P.member_id(member)                                  # the device result was kept: numpy was never asked ...
		assert not torch.equal(U.cpu(), real_host(Wt)), P.member_id(member)           # ... and U is not numpy's
		exact = torch.linalg.pinv(Wt.double())
		err = float((U.cpu().double() - exact).norm() / exact.norm())
		assert err < 1e-6, (P.member_id(member), err)
