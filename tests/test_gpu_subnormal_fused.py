"""Subnormal scores and subnormal operands through the bf16 matrix-core routes: the fused score + top-k on every sweep body (prepass group
maxima -> tau -> ladder -> filter -> select), the small-batch route, the one-pass evaluation and the error sums, ops.sumsq and ops.scale_copy.

The data are integers times a power of two (tests/subnormal_cases.py: all-sub, straddle, sub-in, sums-int), so every product and every partial
sum is exactly representable and the expected bits do not depend on the summation order.  The reference is the IEEE result formed on the host;
a flushed operand (sub-in: every score 0), a flushed sum (all-sub: every score 0, every id a tie) or a threshold flushed to 0 shows as wrong
values, wrong ids, wrong group maxima or a broken ladder invariant.  Nothing is read back from the device to form an expectation; no
tolerance.  Bodies and shapes: fused_exact_cases.BODIES (the smallest I at which the plan takes each body), Q = 130, private 0xff-filled
workspaces with a guard behind them, operands as views into NaN-filled buffers (the helpers of tests/test_gpu_fused_nonfinite.py).

all-sub: the score's bit pattern is |n| < 2^16, so the coarse threshold (the 16-bit key prefix of the k-th group maximum) is +0 for every
query and about half of the row passes it.  On the bodies whose segments cannot hold that many candidates (ladder, staged at k = 100, q16,
wide, and the k = 700 plans in part) a segment overflows and the select repairs by scanning the row: intended, and asserted through the
fallback counter wherever the host counts show that an overflow cannot be avoided.  qt1 and ring at k = 100 have room for 16 512 candidates
per query, twice the row: they cannot overflow, and there the sweep's own count of the candidates it offered is held to the number of items
at or above +0 instead (_check_all_sub_path), so the path a case took is known either way.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import few_numpy as fn  # noqa: E402
import fused_exact_cases as fx  # noqa: E402
import subnormal_cases as sn  # noqa: E402
import test_gpu_fused_nonfinite as tn  # noqa: E402  (its launch helpers; pytest collects none of its tests from here)

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
Q_FUSED = 130
_RUNS = [(b, k) for b in fx.BODIES for k in fx.BODIES[b][3]]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@functools.lru_cache(maxsize=4)
def _case(name, Q, I, K, k, seed=0):
	return sn.IntCase(name, Q, I, K, k, seed=seed)


def _assert_topk(got_v, got_i, want_v, want_i, case, what):
	bad = np.nonzero((sn.bits32(got_v) != sn.bits32(want_v)).any(1) | (got_i != want_i).any(1))[0]
	if bad.size:
		q = int(bad[0])
		j = int(np.nonzero((sn.bits32(got_v[q]) != sn.bits32(want_v[q])) | (got_i[q] != want_i[q]))[0][0])
		raise AssertionError(f"{what}: {bad.size} of {got_v.shape[0]} queries differ (value bits in {int((sn.bits32(got_v) != sn.bits32(want_v)).any(1).sum())}, all returned values zero: "
							 f"{not got_v.any()}); query {q} from rank {j}: got {got_i[q, j:j + 5].tolist()} {[hex(int(b)) for b in sn.bits32(got_v[q, j:j + 5])]}, "
							 f"want {want_i[q, j:j + 5].tolist()} {[hex(int(b)) for b in sn.bits32(want_v[q, j:j + 5])]}")


def _check_ladder(state, S, kth):
	"""The invariants of tests/test_gpu_fused_exact.py on float64 scores: (a) candidates counted at level >= j never outnumber the items that
	score >= levels[j - 1]; (b) tau0 <= tau_final <= the true k-th score; (c) the levels ascend from tau0.  All compares by value, in float64
	on the host (a subnormal level is a number like any other here)."""
	lv, cnt = state["levels"].astype(np.float64), state["counts"].astype(np.int64)
	tf, t0 = state["tau_final"].astype(np.float64), state["tau0"].astype(np.float64)
	assert not np.isnan(lv).any() and not np.isnan(tf).any() and not np.isnan(t0).any()
	assert (np.diff(lv, axis=1) >= 0).all() and (lv[:, 0] >= t0).all(), "(c) levels out of order or below tau0"
	counted_ge = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]
	true_ge = np.stack([(S >= lv[:, j][:, None]).sum(1) for j in range(lv.shape[1])], axis=1)
	over = np.argwhere(counted_ge > true_ge)
	assert over.size == 0, f"(a) query {over[0][0]}, level {over[0][1] + 1}: {counted_ge[tuple(over[0])]} counted >= {lv[tuple(over[0])]}, only {true_ge[tuple(over[0])]} items"
	assert (t0 <= tf).all(), "(b) tau_final below tau0"
	bad = np.nonzero(tf > kth)[0]
	assert bad.size == 0, f"(b) tau_final above the true k-th score: query {bad[0]}: {tf[bad[0]]} > {kth[bad[0]]} (tau0 {t0[bad[0]]})"
	return t0


def _run_fused(ops, body, k, name, leading=False):
	Q = Q_FUSED
	plan, kw, Kp, K, I = tn._plan(ops, body, k, Q, leading)
	case = _case(name, Q, I, K, k)
	Xp, Etp = tn._operands(case, Kp)
	ws, guard = tn._guarded_workspace(ops, plan, Q, I, Kp, k)
	perm = torch.randperm(I, generator=torch.Generator().manual_seed(I + k)) if leading else None
	got_v, got_i, nfb = tn._fused_call(ops, Xp, Etp, I, k, ws, kw, ids=perm.int().cuda() if leading else None)
	what = f"{body} k={k} {name}"
	assert bool((guard == 0xff).all()), f"{what}: bytes written behind the workspace"
	want_v, want_i = case.topk(item_ids=perm.numpy() if leading else None)
	_assert_topk(got_v, got_i, want_v, want_i, case, what)
	# the prepass' group maxima: a flushed v_max or a flushed accumulator shows here first
	gmax, info = ops.fused_group_maxima(ws, Q, I, Kp, k, **kw)
	want_g = case.gmax(fx.sample_tiles(plan, I, leading, plan["lg"] == 4), plan["group"])
	got_g = gmax.cpu().numpy()
	assert got_g.shape == want_g.shape, (got_g.shape, want_g.shape, info)
	assert np.array_equal(sn.bits32(got_g), sn.bits32(want_g)), f"{what}: {int((sn.bits32(got_g) != sn.bits32(want_g)).sum())} of {want_g.size} group maxima differ (all zero: {not got_g.any()})"
	if name != "sub-in":
		assert sn.is_subnormal(want_g).mean() > 0.2
	kth = want_v[:, -1].astype(np.float64)
	if plan["ladder"]:
		t0 = _check_ladder(ops.fused_ladder_state(ws, Q, I, Kp, k, **kw), case.S, kth)
		if name == "sub-in":
			assert (t0 > 0).all(), "tau0 is not above zero although every k-th group maximum is a positive normal number"
	if name == "all-sub":
		_check_all_sub_path(ops, ws, case, plan, Kp, kw, want_g, nfb, what)
	return nfb


def _check_all_sub_path(ops, ws, case, plan, Kp, kw, want_g, nfb, what):
	"""all-sub: which path the call took, from the host scores alone.  The coarse threshold (the 16-bit key prefix of the k-th largest group
	maximum: at most 4096 maxima per query) is +0 for every query, so every item that scores >= 0 is a candidate: about half of the row.
	A query's candidates go into lg x splits segments of segment_capacity entries.  Where the items at or above zero of even one query
	outnumber all of its segments together, a segment must overflow and the select must repair: the fallback counter is not zero.  (It may
	be non-zero below that too: one segment can fill up alone.)  Where no query fell back, nothing overflowed and the sweep's own count of
	the candidates it offered (one stage, no ladder: every offer counted once) must be exactly the number of items at or above +0 -- a
	threshold other than +-0, or a compare that lost the positive subnormals or let the negative ones through, changes that number."""
	Q, I, k = case.Q, case.I, case.k
	assert want_g.shape[1] <= 4096
	tau0 = -np.sort(-want_g.astype(np.float64), axis=1)[:, k - 1].astype(np.float32)
	tau = fx.coarse_floor(tau0)
	assert (tau0 > 0).all() and not sn.bits32(np.ascontiguousarray(tau)).any()      # +0, bit for bit, for every query
	ge = (case.N >= 0).sum(1)
	cap = plan["lg"] * plan["splits"] * plan["segment_capacity"]
	print(f"{what}: {nfb} fallbacks; items at or above +0 per query {ge.min()}..{ge.max()}, room for {cap} candidates per query")
	if ge.max() > cap:
		assert nfb > 0, f"{what}: no query took the repair path although {ge.max()} candidates of one query cannot fit its {cap} segment entries"
	if nfb == 0 and not plan["ladder"]:
		surv = ops.fused_survivors(ws, Q, I, Kp, k, **kw) * Q
		assert abs(surv - round(surv)) < 1e-3 and int(round(surv)) == int(ge.sum()), f"{what}: the sweep offered {surv} candidates, {int(ge.sum())} items score at or above +0"


# ------------------------------------------------------------------ 3. every case on every body
@pytest.mark.parametrize("name", sn.INT_CASES)
@pytest.mark.parametrize("body,k", _RUNS, ids=[f"{b}-k{k}" for b, k in _RUNS])
def test_fused_topk_on_subnormal_scores_and_operands(ops, body, k, name):
	_run_fused(ops, body, k, name)


@pytest.mark.parametrize("name", ["straddle"])
def test_leading_sample_and_permuted_item_ids(ops, name):
	_run_fused(ops, "ladder", 100, name, leading=True)


# ------------------------------------------------------------------ 5. the small-batch route
def _few_queries(Kp):
	return (1, 17, 64) if Kp <= 256 else (1, 17, 48)      # (Kp = 640 stages at most 48 query rows: ops.score_topk_few_ok)


@pytest.mark.parametrize("name", sn.INT_CASES)
@pytest.mark.parametrize("Kp", [64, 256, 640])
def test_small_batch_rows_and_topk(ops, Kp, name):
	"""ops.score_rows_few: every score and every maximum of 64 consecutive items, bit for bit; ops.score_topk_few: values and ids."""
	I, k, K = 4101, 100, Kp - 7
	for Q in _few_queries(Kp):
		assert ops.score_topk_few_ok(Q, I, Kp, k)
		case = _case(name, Q, I, K, k)
		Xp, Etp = tn._operands(case, Kp)
		S32 = case.values32()
		got_S, got_GM = ops.score_rows_few(Xp, Etp, I)
		torch.cuda.synchronize()
		gs = got_S.cpu().numpy()
		assert np.array_equal(sn.bits32(gs), sn.bits32(S32)), f"Q={Q} Kp={Kp} {name}: {(sn.bits32(gs) != sn.bits32(S32)).mean():.2f} of the scores differ (all zero: {not gs.any()})"
		assert np.array_equal(sn.bits32(got_GM.cpu().numpy()), sn.bits32(fn.group_maxima(S32))), f"Q={Q} Kp={Kp} {name}: group maxima"
		ws = ops.few_workspace(Q, I, Kp, k, torch.device("cuda"))
		ws.fill_(0xff)
		got = ops.score_topk_few(Xp, Etp, I, k, workspace=ws)
		torch.cuda.synchronize()
		want_v, want_i = case.topk()
		_assert_topk(got.values.cpu().numpy(), got.indices.cpu().numpy().astype(np.int64), want_v, want_i, case, f"few Q={Q} Kp={Kp} {name}")


@pytest.mark.parametrize("name", sn.INT_CASES)
@pytest.mark.parametrize("Kp", [64, 256])
def test_small_batch_equals_fused_on_the_same_operands(ops, Kp, name):
	"""The header's parity claim at Kp <= 256, on the same device operands, both routes held to the host reference (I = 8209: the smallest the
	fused route takes)."""
	Q, I, k, K = 17, 8209, 100, Kp - 7
	assert ops.fused_supported(Q, I, Kp, k) and ops.score_topk_few_ok(Q, I, Kp, k)
	case = _case(name, Q, I, K, k)
	Xp, Etp = tn._operands(case, Kp)
	want_v, want_i = case.topk()
	few = ops.score_topk_few(Xp, Etp, I, k)
	fv, fi = few.values.cpu().numpy(), few.indices.cpu().numpy().astype(np.int64)
	fused = ops.score_topk_fused(Xp, Etp, I, k, workspace=fx.poisoned_workspace(ops, Q, I, Kp, k))
	torch.cuda.synchronize()
	uv, ui = fused.values.cpu().numpy(), fused.indices.cpu().numpy().astype(np.int64)
	_assert_topk(fv, fi, want_v, want_i, case, f"few Kp={Kp} {name}")
	_assert_topk(uv, ui, want_v, want_i, case, f"fused Kp={Kp} {name}")


# ------------------------------------------------------------------ 4. the error sums in the subnormal range
def _exact_matrix(A):
	"""A [Q x I] (bf16-exact float64) as a view [1 : Q + 1, 8 : 8 + I] of a NaN-filled bf16 buffer with a row pitch that is a multiple of 8."""
	Q, I = A.shape
	buf = torch.full((Q + 2, tn._ceil32(I) + 16), float("nan"), dtype=BF16)
	buf[1:Q + 1, 8:8 + I] = sn.to_bf16_exact(A)
	Ad = buf.cuda()[1:Q + 1, 8:8 + I]
	assert Ad.data_ptr() % 16 == 0 and Ad.stride(0) % 8 == 0
	return Ad


def _assert_sums(err, nrm, case, what):
	for got, want, label in ((err, case.err(), "err_sq"), (nrm, case.nrm(), "norm_sq")):
		g = sn.bits32(got.cpu().numpy())
		assert np.array_equal(g, sn.bits32(want)), f"{what}: {label} differs in {int((g != sn.bits32(want)).sum())} of {want.size} rows (all zero: {not g.any()}); first got {hex(int(g[0]))} want {hex(int(sn.bits32(want)[0]))}"


@pytest.mark.parametrize("Kp", [64, 128, 256])
def test_error_sums_of_subnormal_squares(ops, Kp):
	"""anncur_approx_error, anncur_approx_error_packed (I = 4101, a ragged tail) and anncur_eval_fused (I = 8209: the smallest cell its plan
	takes) on sums-int: S_hat = n 2^-70, A = (n + delta) 2^-70; every (S_hat - A)^2 and every A^2 is a subnormal, err^2 = sum delta^2 2^-140
	stays one, norm^2 crosses into the normal range; every partial sum in any order is exact.  A flushed square gives 0 for both sums."""
	Q, k = 130, 100
	for I, routes in ((4101, ("approx_error", "approx_error_packed")), (8209, ("eval_fused",))):
		case = sn.SumsIntCase(Q, I, Kp - 8, seed=1)
		Xp, Etp = tn._operands(case, Kp)
		Ad = _exact_matrix(case.A)
		for route in routes:
			if route == "approx_error":
				err, nrm = ops.approx_error(Xp, Etp[:I], Ad)
			elif route == "approx_error_packed":
				assert ops.approx_error_packed_ok(Kp, Ad)
				err, nrm = ops.approx_error_packed(Xp, Etp, Ad, I)
			else:
				assert ops.eval_fused_ok(Kp, Ad, Q, I, k)
				top, err, nrm = ops.eval_fused(Xp, Etp, Ad, I, k)
				val, rows = fx.reference_topk(torch.from_numpy(case.N), k)
				want_v = (val.numpy().astype(np.float64) * 2.0 ** sn.SUMS_INT_E).astype(np.float32)
				torch.cuda.synchronize()
				_assert_topk(top.values.cpu().numpy(), top.indices.cpu().numpy().astype(np.int64), want_v, rows.numpy(), case, f"eval_fused Kp={Kp}")
			torch.cuda.synchronize()
			_assert_sums(err, nrm, case, f"{route} Kp={Kp} I={I}")


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "atomics"])
@pytest.mark.parametrize("M,N", [(130, 4101), (1, 77), (257, 33)])
def test_sumsq_of_subnormal_squares(ops, M, N, ordered):
	"""ops.sumsq (anncur_sumsq_ordered / anncur_sumsq) on a = ints 2^-70 (|int| <= 5): every square a subnormal, the sum m 2^-140 with m < 2^24,
	exact in any order; rows pitched inside a NaN-filled buffer."""
	a = np.random.default_rng([M, N]).integers(-5, 6, (M, N))
	units = int((a * a).sum())
	assert 0 < units < 1 << 24
	want = np.array([units * 2.0 ** -140], dtype=np.float64).astype(np.float32)
	assert float(want[0]) == units * 2.0 ** -140
	buf = torch.full((M + 2, N + 5), float("nan"), dtype=F32, device="cuda")
	v = buf[1:M + 1, 2:N + 2]
	v.copy_(torch.from_numpy((a * 2.0 ** -70).astype(np.float32)))
	out = torch.full((1,), float("nan"), dtype=F32, device="cuda")
	ops.sumsq(v, out=out, ordered=ordered)
	got = sn.bits32(out.cpu().numpy())
	assert got[0] == sn.bits32(want)[0], f"got {hex(int(got[0]))}, want {hex(int(sn.bits32(want)[0]))} ({units} units of 2^-140)"


@pytest.mark.parametrize("alpha,divide_by", [(2.0 ** -45, None), (1.0, 2.0 ** 45), (2.0 ** -100, 2.0 ** 40), (2.0 ** -140, None), (-2.0 ** 20, 2.0 ** 65)])
def test_scale_copy_into_the_subnormal_range(ops, alpha, divide_by):
	"""dst = alpha / divide_by[0] * src with powers of two: the factor (2^-45 or 2^-140: the second a subnormal itself, and the quotient of
	two normal numbers in the third case) and every result are exactly representable, the results subnormal.  A division or a product
	that flushes gives zeros.  src and dst are strided views (a scaled transpose) inside NaN / poison-filled buffers."""
	M, N = 33, 130
	f = alpha / (divide_by if divide_by is not None else 1.0)
	e_src = -100 if abs(f) == 2.0 ** -45 else 0
	m = np.random.default_rng(3).integers(-(1 << 11) + 1, 1 << 11, (M, N))
	src = (m * 2.0 ** e_src).astype(np.float32)
	want64 = src.astype(np.float64) * f
	want = want64.astype(np.float32)
	assert (want.astype(np.float64) == want64).all() and sn.is_subnormal(want)[m != 0].all() and (m != 0).mean() > 0.99
	sbuf = torch.full((M + 2, 2 * N + 3), float("nan"), dtype=F32, device="cuda")
	s = sbuf[1:M + 1, 1:1 + 2 * N:2]
	s.copy_(torch.from_numpy(src))
	dbuf = torch.full((N + 2, M + 5), 0x7fc00123, dtype=torch.int32, device="cuda")
	d = dbuf.view(F32)[1:N + 1, 2:M + 2].t()
	div = torch.tensor([divide_by], dtype=F32, device="cuda") if divide_by is not None else None
	ops.scale_copy(s, d, alpha=alpha, divide_by=div)
	exp = torch.full((N + 2, M + 5), 0x7fc00123, dtype=torch.int32)
	exp[1:N + 1, 2:M + 2] = torch.from_numpy(want.view(np.int32)).t()
	got = dbuf.cpu()
	assert torch.equal(got, exp), f"{int((got != exp).sum())} words differ (all results zero: {not bool(d.cpu().any())})"
