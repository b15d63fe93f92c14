"""NaN and +-inf scores through the fused score + top-k on every sweep body, the one-pass evaluation, the error kernels, the dense route,
a bf16 FlatIPIndex and the split-bf16 route.  include/anncur_hip.h: "NaN scores are never selected"; -inf scores are ordinary candidates; a
row with fewer than k non-NaN scores is padded with (-inf, -1).

The reference is the host module tests/nonfinite_cases.py (classes by exact indicator products, THE top-k with NaN left out), never another
device route -- except the split route, which must equal ops.score_topk_dense on the same fp32 operands, and the dense route is held to the
host reference first (test_dense_route_equals_the_reference).  No tolerance anywhere: value bits and ids.

Cases (nonfinite_cases.Case; built from the plan's own sample so that plants land inside and outside it): nan-items, nan-queries,
inf-column (|J| = 3 and k + 3), neg-inf-floor, inf-minus-inf, few-left (Q = 5: every query takes the select's whole-row rescan), mixed, and
nan-tiles (whole sampled tiles NaN: k - 10 of the group maxima are NaN and k numbers are left).
Bodies: for Kp <= 256 the ladder default, staged, mfma32 and qt1 at k = 100 (wave-level select) and k = 700 (workgroup-level select);
Kp = 512 default (scoreq16_kernel) and mfma32 (the ring body); the wide kernel at Kp = 640.  Shapes: the smallest I at which the plan query
reports the body, plus a ragged tail of 17 (_BODY).  Every call runs on a private workspace filled with 0xff, outputs pre-filled with a
sentinel and operands that are views into NaN-filled buffers.

What a NaN row does (read from the kernels, then seen here): the prepass' fmaxf chains skip NaN, an all-NaN group's maximum is NaN,
kth_value_wave_kernel keys it as 0; with fewer than k non-NaN maxima tau0 is NaN, every filter `v >= tau` is false, the sweep offers
nothing, and select_candidates_kernel / select_wave_kernel rescan the whole row (the fallback counter counts it).  A k-th maximum of -inf
also comes out of the coarse threshold kernel as a NaN (the 16-bit prefix of -inf's key is a NaN pattern): the same path.

The padded rows.  A sweep lane past Q carries the threshold +inf and a real query's operand row, so a +inf score of the block's last query
passes `v >= tau` there; the candidate region holds Q rows and is the workspace's last, so a store from such a lane would land behind the
workspace.  The sweeps start those lanes' candidate counts at PAD_ROW_COUNT (csrc/common.hpp), which every store's capacity check refuses.
inf-column and neg-inf-floor give query Q - 1 its +inf scores, and every call here runs with a guard of 0xff behind its workspace that must
come back untouched (_guarded_workspace).

Mutations (each a build of its own loaded through ANNCUR_LIB, on an MI355X):
  1. sel_finish and wsel_finish pad with (0, 0) instead of (-inf, -1): every padded case fails (nan-queries, neg-inf-floor, few-left and mixed
     on every body, route and Kp: 66 tests), every other test passes.
  2. every sweep filter `v >= tau` as `!(v < tau)`: nan-items fails through the survivor count (31 264 candidates offered, at most 30 984
     items at or above the thresholds) -- the returned top-k alone does not show it.  The negated compare also lets the padded lanes
     (tau = +inf) take NaN scores, which that build stored out of bounds: its later cases say nothing.
  3. kth_value_wave_kernel keys a NaN maximum as f32_sortable(v) instead of 0: no test fails, and none can.  The matrix cores return the
     NaN 0xffc00000 for NaN operands of either sign (pinned in _check_nan_items_sweep), and its sortable key 0x003fffff already lies below
     -inf's 0x007fffff: both builds order the keys alike, and with fewer than k numbers tau0 unsorts to a NaN either way.  nan-tiles covers
     the one place where they could differ (NaN maxima beside at least k numbers: a NaN keyed ABOVE the numbers would put tau0 near the 4th
     largest maximum, above the true k-th score: nfb == 0 and the ladder's tau0 bound would fail).  The `? : 0` guards against a positive
     NaN, which nothing upstream of the kernel produces.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_exact_cases as fx  # noqa: E402
import nonfinite_cases as nf  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAN, INF = nf.NAN, nf.INF
SENTINEL_V, SENTINEL_I = 12345.0, -7

_BODY = fx.BODIES   # body -> (Kp, logical K, flags, {k: (I, lg, QT, ladder, stage_pred)}): shared with tests/test_gpu_subnormal_exact.py
_RUNS = [(b, k) for b in _BODY for k in _BODY[b][3]]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _ceil32(n):
	return -(-n // 32) * 32


def _plan(ops, body, k, Q, leading=False):
	Kp, K, flags, per_k = _BODY[body]
	I, lg, QT, ladder, pred = per_k[k]
	kw = dict(flags, leading_sample=leading)
	plan = ops.fused_plan(Q, I, Kp, k, **kw)
	assert (plan["lg"], plan["QT"], plan["ladder"], plan["stage_pred"], plan["n_stages"]) == (lg, QT, ladder, [pred], 1), plan
	assert plan["n_tiles"] == -(-I // (256 if lg == 4 else 32)), plan
	return plan, kw, Kp, K, I


@functools.lru_cache(maxsize=4)
def _case(name, Q, I, K, k, sampled, x_nnz=None):
	return nf.Case(name, Q, I, K, k, np.array(sampled), x_nnz=x_nnz)


def _bf16(a):
	t = torch.from_numpy(np.ascontiguousarray(a)).to(BF16)
	back = t.double().numpy()
	assert ((back == a) | (np.isnan(back) & np.isnan(a))).all()   # bf16-exact operands
	return t


def _operands(case, Kp):
	"""Packed bf16 operands as views into NaN-filled buffers: Xp [Q x Kp] with ldx = Kp + 16, a NaN row before and after and NaN between the
	rows; Etp [ceil32(I) x Kp] with 32 NaN rows before and after (rows I .. ceil32(I) - 1 and columns K .. Kp - 1 are zero: the operand contract)."""
	Q, K, I = case.Q, case.K, case.I
	xb = torch.full((Q + 2, Kp + 16), NAN, dtype=BF16)
	xb[1:Q + 1, :Kp] = 0
	xb[1:Q + 1, :K] = _bf16(case.X)
	Ip = _ceil32(I)
	eb = torch.full((Ip + 64, Kp), NAN, dtype=BF16)
	eb[32:32 + Ip] = 0
	eb[32:32 + I, :K] = _bf16(case.E.T)
	Xp, Etp = xb.cuda()[1:Q + 1, :Kp], eb.cuda()[32:32 + Ip]
	assert Xp.stride(0) == Kp + 16 and Etp.is_contiguous()
	return Xp, Etp


def _guarded_workspace(ops, plan, Q, I, Kp, k):
	"""A private workspace filled with 0xff with a guard of 0xff behind it -> (workspace view of exactly the bytes the library asks for, guard view).
	The candidate segments are the workspace's last region and hold Q rows; a sweep lane past Q (the row blocks are padded to BQ rows) that
	stored a candidate would write behind the workspace.  The guard is large enough to take every such store (twice the padded rows'
	segments), so a library that does store there shows it as a changed guard byte and writes nothing outside this buffer."""
	from anncur_amd import _lib
	nbytes = _lib.load().anncur_score_topk_workspace_bytes(Q, I, Kp, k)
	BQ = 256 if plan["lg"] == 4 else 128 * plan["QT"]
	guard = 2 * (-(-Q // BQ) * BQ - Q) * plan["lg"] * plan["splits"] * plan["segment_capacity"] * 8 + (1 << 20)
	buf = torch.full((nbytes + guard + 256,), 0xff, dtype=torch.uint8, device="cuda")
	off = (-buf.data_ptr()) % 256
	return buf[off:off + nbytes], buf[off + nbytes:]


def _fused_call(ops, Xp, Etp, I, k, ws, kw, ids=None):
	"""ops.score_topk_fused with outputs this test allocates and pre-fills (the wrapper allocates its own): -> (values, ids, nfb) on the host."""
	from anncur_amd import _lib
	Q, Kp = Xp.shape
	val = torch.full((Q, k), SENTINEL_V, dtype=F32, device="cuda")
	idx = torch.full((Q, k), SENTINEL_I, dtype=torch.int32, device="cuda")
	nbytes = _lib.load().anncur_score_topk_workspace_bytes(Q, I, Kp, k)
	assert 0 < nbytes <= ws.numel() and ws.data_ptr() % 256 == 0 and Etp.is_contiguous() and Etp.shape[0] >= _ceil32(I)
	ops.check(_lib.load().anncur_score_topk_ex(ops._p(Xp), ops._ld(Xp), ops._p(Etp), Kp, Q, I, Kp, k, ops._p(val), ops._p(idx), ops._p(ws), nbytes,
											   ops._topk_flags(**kw), ops._p(ids) if ids is not None else None, ops._stream()), "score_topk")
	torch.cuda.synchronize()
	return val.cpu().numpy(), idx.cpu().numpy().astype(np.int64), int(ws[:4].view(torch.int32).item())


def _assert_topk(got_v, got_i, S, k, I, item_ids=None, what=""):
	"""Value bits and ids against THE top-k of the reference; never a NaN; pads exactly (-inf, -1) and only at the end of a row."""
	want_v, want_i, n_valid = nf.reference_topk(S, k, item_ids)
	assert not np.isnan(got_v).any(), f"{what}: {int(np.isnan(got_v).sum())} NaN values returned (first in query {int(np.argwhere(np.isnan(got_v))[0][0])})"
	pad = got_i < 0
	assert (got_i[pad] == -1).all() and (got_v[pad] == -INF).all(), f"{what}: a pad that is not (-inf, -1)"
	assert (pad == (np.arange(k)[None, :] >= n_valid[:, None])).all(), f"{what}: pads elsewhere than behind the row's {n_valid.min()}..{n_valid.max()} non-NaN scores"
	assert (got_i[~pad] < I).all()
	bad = np.nonzero((got_v.view(np.uint32) != want_v.view(np.uint32)).any(1) | (got_i != want_i).any(1))[0]
	if bad.size:
		q = int(bad[0])
		j = int(np.nonzero((got_v[q].view(np.uint32) != want_v[q].view(np.uint32)) | (got_i[q] != want_i[q]))[0][0])
		raise AssertionError(f"{what}: {bad.size} queries differ (first {bad[:8].tolist()}); query {q} from rank {j}: got {got_i[q, j:j + 6].tolist()} {got_v[q, j:j + 6].tolist()}, "
							 f"want {want_i[q, j:j + 6].tolist()} {want_v[q, j:j + 6].tolist()} ({int(n_valid[q])} non-NaN scores)")
	return want_v, want_i, n_valid


def _ge(a, b):
	"""a >= b with NaN below everything, not even >= itself as a level (a NaN level is reached by nothing)."""
	with np.errstate(invalid="ignore"):
		return np.where(np.isnan(a) | np.isnan(b), False, a >= b)


def _check_ladder(state, S, kth):
	"""_check_ladder of tests/test_gpu_fused_exact.py on the queries with at least k non-NaN scores (kth not NaN), NaN below every level:
	  (a) for every level j, the candidates counted at level >= j never outnumber the items that truly score >= levels[j - 1];
	  (b) tau0 <= tau_final <= the true k-th score;  (c) the levels ascend and start at or above tau0
	-- (b) and (c) where tau0 is a number; where it is a NaN (fewer than k non-NaN group maxima, or a k-th maximum of -inf) the levels are NaN,
	nothing may be counted against them, and tau_final is a NaN or at most the k-th score.  tau0 itself: a NaN or at most the k-th score."""
	has_k = ~np.isnan(kth)
	lv = state["levels"].astype(np.float64)
	cnt = state["counts"].astype(np.int64)
	with np.errstate(invalid="ignore"):
		tf, t0 = state["tau_final"].astype(np.float64), state["tau0"].astype(np.float64)
	num = has_k & ~np.isnan(t0)
	with np.errstate(invalid="ignore"):
		assert (np.isnan(t0[has_k]) | (t0[has_k] <= kth[has_k])).all(), "tau0 above the true k-th non-NaN score"
		assert (np.isnan(tf[has_k]) | (tf[has_k] <= kth[has_k])).all(), f"(b) tau_final above the true k-th score: queries {np.nonzero(has_k & (tf > kth))[0][:8].tolist()}"
		assert (lv[num, 1:] >= lv[num, :-1]).all() and (lv[num, 0] >= t0[num]).all(), "(c) levels out of order or below tau0"
		assert (t0[num] <= tf[num]).all(), "(b) tau_final below tau0"
	counted_ge = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]
	true_ge = np.stack([_ge(S, lv[:, j][:, None]).sum(1) for j in range(lv.shape[1])], axis=1)
	over = np.argwhere((counted_ge > true_ge) & has_k[:, None])
	assert over.size == 0, f"(a) query {over[0][0]}, level {over[0][1] + 1}: {counted_ge[tuple(over[0])]} counted >= {lv[tuple(over[0])]}, only {true_ge[tuple(over[0])]} items"


def _check_nan_items_sweep(ops, ws, case, plan, Kp, kw, nfb, kth):
	"""nan-items and nan-tiles only (every score outside the NaN items is a finite integer; no segment can overflow): nfb == 0, the prepass' group
	maxima against the host scores (fmaxf skips a NaN cell; an all-NaN group's maximum is a NaN), and the survivor count of _check_sweep in tests/test_gpu_fused_kp512_wide_exact.py under its
	preconditions -- one stage, every offer counted: sum_q #{i : S[q, i] >= tau[q]}, NaN never >= anything; tau = tau0 cut to its 16-bit key
	prefix (at most 4096 group maxima).  Under the ladder the thresholds rise in-launch from tau to at most the k-th score: the count lies
	between the items at or above the k-th score and that sum."""
	Q, I, k, S = case.Q, case.I, case.k, case.S
	assert nfb == 0, f"{nfb} queries fell back: a NaN cost them candidates"
	gmax, info = ops.fused_group_maxima(ws, Q, I, Kp, k, **kw)
	want = nf.nan_ignoring_gmax(S, fx.sample_tiles(plan, I, kw["leading_sample"], plan["lg"] == 4), fx.group_rows(plan["group"]))
	got = gmax.cpu().double().numpy()
	assert got.shape == want.shape and info["n_groups"] <= 4096, (info, got.shape, want.shape)
	same = (got == want) | (np.isnan(got) & np.isnan(want))
	assert same.all(), f"{int((~same).sum())} group maxima differ from the maximum of the non-NaN cells"
	assert np.isnan(want).any() == (case.name == "nan-tiles")
	# the only NaN the threshold kernel ever sees: the matrix cores' 0xffc00000, whose sortable key 0x003fffff lies below -inf's -- which is why
	# kth_value_wave_kernel's `? : 0` changes nothing today (a positive NaN would rank above every number without it)
	nan_bits = np.unique(gmax.cpu().numpy().view(np.uint32)[np.isnan(got)])
	assert nan_bits.size == 0 or nan_bits.tolist() == [0xffc00000], [hex(int(b)) for b in nan_bits]
	tau0 = nf.kth_largest_nan_lowest(want, k)
	assert (tau0 <= kth).all()
	tau = fx.coarse_floor(tau0.astype(np.float32)).astype(np.float64)
	assert (tau <= tau0).all()
	hi = int(_ge(S, tau[:, None]).sum())
	lo = int(_ge(S, kth[:, None]).sum())
	surv = ops.fused_survivors(ws, Q, I, Kp, k, **kw) * Q
	assert abs(surv - round(surv)) < 1e-3
	surv = int(round(surv))
	if plan["ladder"]:
		assert lo <= surv <= hi, f"ladder sweep: {surv} candidates offered, outside [{lo}, {hi}]"
	else:
		assert surv == hi, f"the sweep offered {surv} candidates, {hi} items score at or above the thresholds (a NaN cell offered, or an item lost)"


def _run_case(ops, body, k, name, leading=False):
	Q = nf.case_queries(name)
	plan, kw, Kp, K, I = _plan(ops, body, k, Q, leading)
	sampled = fx.sample_tiles(plan, I, leading, plan["lg"] == 4)
	case = _case(name, Q, I, K, k, tuple(int(t) for t in sampled))
	Xp, Etp = _operands(case, Kp)
	ws, guard = _guarded_workspace(ops, plan, Q, I, Kp, k)
	perm = torch.randperm(I, generator=torch.Generator().manual_seed(I + k)) if leading else None
	got_v, got_i, nfb = _fused_call(ops, Xp, Etp, I, k, ws, kw, ids=perm.int().cuda() if leading else None)
	assert bool((guard == 0xff).all()), f"{body} k={k} {name}: {int((guard != 0xff).sum())} bytes written behind the workspace (first at +{int((guard != 0xff).nonzero()[0])})"
	want_v, want_i, n_valid = _assert_topk(got_v, got_i, case.S, k, I, perm.numpy() if leading else None, what=f"{body} k={k} {name}")
	rows = got_i if perm is None else np.where(got_i >= 0, np.argsort(perm.numpy())[np.maximum(got_i, 0)], -1)
	if case.nan_items.size:
		assert not np.isin(rows, case.nan_items).any()
	if case.nan_queries.size:
		assert (got_i[case.nan_queries] == -1).all()
	kth = nf.kth_non_nan(case.S, k)
	if plan["ladder"]:
		_check_ladder(ops.fused_ladder_state(ws, Q, I, Kp, k, **kw), case.S, kth)
	if name == "few-left":
		assert nfb == Q, f"few-left: {nfb} of {Q} queries took the whole-row rescan"
	if name in ("nan-items", "nan-tiles"):
		_check_nan_items_sweep(ops, ws, case, plan, Kp, kw, nfb, kth)


# ------------------------------------------------------------------ 1. every case on every body
@pytest.mark.parametrize("name", nf.CASES)
@pytest.mark.parametrize("body,k", _RUNS, ids=[f"{b}-k{k}" for b, k in _RUNS])
def test_fused_topk_with_nan_and_inf_scores(ops, body, k, name):
	_run_case(ops, body, k, name)


@pytest.mark.parametrize("name", nf.CASES)
def test_leading_sample_and_permuted_item_ids(ops, name):
	"""The index builder's hints on the ladder body: the prepass samples the leading tiles, the ids are item_ids[row], ties stay ordered by row."""
	_run_case(ops, "ladder", 100, name, leading=True)


# ------------------------------------------------------------------ 2. the dense route (held to the host reference: the split route is compared with it below)
def _dense_case(ops, name, x_nnz=None, K=56, Kp=64):
	Q, I, k = nf.case_queries(name), 8209, 100
	plan = ops.fused_plan(Q, I, Kp, k)
	return _case(name, Q, I, K, k, tuple(int(t) for t in fx.sample_tiles(plan, I, False, False)), x_nnz)


@pytest.mark.parametrize("name", nf.CASES)
def test_dense_route_equals_the_reference(ops, name):
	case = _dense_case(ops, name)
	X = torch.from_numpy(case.X).float().cuda()
	Et = torch.from_numpy(np.ascontiguousarray(case.E.T)).float().cuda()
	v, i = ops.score_topk_dense(X, Et, case.k)
	torch.cuda.synchronize()
	_assert_topk(v.cpu().numpy(), i.cpu().numpy().astype(np.int64), case.S, case.k, case.I, what=f"dense {name}")


# ------------------------------------------------------------------ 3. one-pass evaluation and the error kernels
def _exact_matrix(case, seed, plant=False):
	"""A = the finite part of S + delta, delta in [-1, 1] (integers, bf16-exact), as a view [1 : Q + 1, 8 : 8 + I] of a NaN-filled bf16 buffer
	with a row pitch that is a multiple of 8.  plant: a -inf and a NaN in A itself (rows 1 and 2)."""
	g = np.random.default_rng(seed)
	A = np.where(np.isfinite(case.S), case.S, 0.0) + g.integers(-1, 2, case.S.shape)
	if plant:
		A[1, case.I // 2], A[2, 5] = -INF, NAN
	assert np.abs(A[np.isfinite(A)]).max() <= 256
	buf = torch.full((case.Q + 2, _ceil32(case.I) + 16), NAN, dtype=BF16)
	buf[1:case.Q + 1, 8:8 + case.I] = _bf16(A)
	Ad = buf.cuda()[1:case.Q + 1, 8:8 + case.I]
	assert Ad.data_ptr() % 16 == 0 and Ad.stride(0) % 8 == 0
	return A, Ad


def _assert_sums(err, nrm, case, A, what):
	want_e, want_n = nf.reference_error_sums(case.S, A)
	ge, gn = err.cpu().numpy(), nrm.cpu().numpy()
	for got, want, label in ((ge, want_e, "err_sq"), (gn, want_n, "norm_sq")):
		nan, inf = np.isnan(want), want == INF
		assert (np.isnan(got) == nan).all(), f"{what}: {label} NaN in rows {np.nonzero(np.isnan(got))[0][:8].tolist()}, the reference in {np.nonzero(nan)[0][:8].tolist()}"
		assert (got[inf] == INF).all(), f"{what}: {label} not +inf in rows {np.nonzero(inf & (got != INF))[0][:8].tolist()}"
		fin = ~nan & ~inf
		assert (got[fin].view(np.uint32) == want[fin].astype(np.float32).view(np.uint32)).all(), f"{what}: {label} differs in a row of finite cells"
	return want_e


@pytest.mark.parametrize("name", nf.CASES + ("nan-items/A",))
@pytest.mark.parametrize("Kp", [64, 128, 256])
def test_eval_fused_and_error_kernels_with_nan_and_inf_scores(ops, Kp, name):
	"""ops.eval_fused (top-k + both sums from one sweep), ops.approx_error_packed and ops.approx_error on the same operands.  X has six
	non-zero columns per query besides the planted ones, so that every sum stays an exact integer below 2^24.  err_sq by class where the row
	holds a non-finite cell (of S_hat - A), bit for bit elsewhere; norm_sq from A alone.  "/A": a -inf and a NaN in the exact matrix itself."""
	from anncur_amd import _lib
	plant = name.endswith("/A")
	case = _dense_case(ops, name[:-2] if plant else name, x_nnz=6, K=Kp - 8, Kp=Kp)
	Q, I, k = case.Q, case.I, case.k
	assert ops.eval_fused_plan(Q, I, Kp, k)["stage_pred"] == [6]
	Xp, Etp = _operands(case, Kp)
	A, Ad = _exact_matrix(case, Kp, plant)
	assert ops.eval_fused_ok(Kp, Ad, Q, I, k)
	nbytes = _lib.load().anncur_eval_fused_workspace_bytes(Q, I, Kp, k)
	buf = torch.full((nbytes + 256,), 0xff, dtype=torch.uint8, device="cuda")   # a private workspace, poisoned
	ws = buf[(-buf.data_ptr()) % 256:][:nbytes]
	val = torch.full((Q, k), SENTINEL_V, dtype=F32, device="cuda")
	idx = torch.full((Q, k), SENTINEL_I, dtype=torch.int32, device="cuda")
	err = torch.full((Q,), SENTINEL_V, dtype=F32, device="cuda")
	nrm = torch.full((Q,), SENTINEL_V, dtype=F32, device="cuda")
	ops.check(_lib.load().anncur_eval_fused_ex(ops._p(Xp), ops._ld(Xp), ops._p(Etp), Kp, None, ops._p(Ad), ops._dt(Ad), ops._ld(Ad), Q, I, Kp, k,
											   ops._p(val), ops._p(idx), ops._p(err), ops._p(nrm), ops._p(ws), nbytes, ops._stream()), "eval_fused")
	torch.cuda.synchronize()
	_assert_topk(val.cpu().numpy(), idx.cpu().numpy().astype(np.int64), case.S, k, I, what=f"eval_fused Kp={Kp} {name}")
	_assert_sums(err, nrm, case, A, f"eval_fused Kp={Kp} {name}")
	lib, st = _lib.load(), ops._stream()
	assert ops.approx_error_packed_ok(Kp, Ad)
	err.fill_(SENTINEL_V), nrm.fill_(SENTINEL_V)
	ops.check(lib.anncur_approx_error_packed(ops._p(Xp), ops._ld(Xp), ops._p(Etp), ops._ld(Etp), ops._p(Ad), ops._dt(Ad), ops._ld(Ad), Q, I, Kp,
											 ops._p(err), ops._p(nrm), st), "approx_error_packed")
	_assert_sums(err, nrm, case, A, f"approx_error_packed Kp={Kp} {name}")
	err.fill_(SENTINEL_V), nrm.fill_(SENTINEL_V)
	Et = Etp[:I]
	ops.check(lib.anncur_approx_error(ops._p(Xp), ops._dt(Xp), ops._ld(Xp), ops._p(Et), ops._dt(Et), ops._ld(Et), ops._p(Ad), ops._dt(Ad), ops._ld(Ad), Q, I, Kp,
									  ops._p(err), ops._p(nrm), st), "approx_error")
	_assert_sums(err, nrm, case, A, f"approx_error Kp={Kp} {name}")


# ------------------------------------------------------------------ 4. a bf16 FlatIPIndex with one corrupt embedding
def test_flat_ip_index_bf16_never_returns_an_item_with_a_nan_embedding(ops):
	"""Item j has a NaN in its embedding: every query is answered as by the index built without item j (ids mapped), and j never appears.
	The index keeps its rows in norm-bucket order (the NaN norm moves the bucket bounds, so the two indexes order their rows differently)
	and ties are ordered by ROW: each index is held to THE top-k of the host scores in its own row order (its row -> id map, index._ids),
	value bits and ids; the two answers then hold the same value bits, and the same ids wherever no tie is involved."""
	from anncur_amd.nearest_nbr import FlatIPIndex
	d, n, nq, k, j = 56, 8209, 70, 100, 4321
	g = np.random.default_rng(4)
	emb = g.integers(-3, 4, (n, d)).astype(np.float32)
	xq = g.integers(-2, 4, (nq, d)).astype(np.float32)
	assert ops.fused_supported(nq, n, ops.padded_k(d), k) and ops.fused_supported(nq, n - 1, ops.padded_k(d), k)
	bad = emb.copy()
	bad[j, 9] = NAN
	S = nf.scores(xq.astype(np.float64), bad.T.astype(np.float64))
	assert np.isnan(S[:, j]).all() and np.isnan(S).sum() == nq
	got = []
	for vecs, Sx in ((bad, S), (np.delete(emb, j, axis=0), np.delete(S, j, axis=1))):
		index = FlatIPIndex(d, dtype="bf16")
		index.add(vecs)
		D, Ix = index.search(xq, k)
		perm = index._ids.cpu().numpy().astype(np.int64)            # row of the packed operand -> id
		assert np.array_equal(np.sort(perm), np.arange(vecs.shape[0]))
		want_v, want_i, n_valid = nf.reference_topk(Sx[:, perm], k, item_ids=perm)
		assert (n_valid >= k).all()
		assert np.array_equal(D.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(Ix, want_i), f"index of {vecs.shape[0]} vectors differs from THE top-k in its row order"
		got.append((D, Ix))
	(Da, Ia), (Db, Ib) = got
	Ib = Ib + (Ib >= j)
	assert not (Ia == j).any()
	assert np.array_equal(Da.view(np.uint32), Db.view(np.uint32))
	untied = np.ones_like(Da, dtype=bool)
	untied[:, 1:] &= Da[:, 1:] != Da[:, :-1]
	untied[:, :-1] &= Da[:, :-1] != Da[:, 1:]
	untied[:, -1] = False                                            # (the k-th value may tie with items outside the result)
	assert (Ia[untied] == Ib[untied]).all() and untied.sum() > nq


# ------------------------------------------------------------------ 5. the split-bf16 route
def _split_operands(ops, case, seed):
	"""fp32 operands with non-zero low parts (nonfinite_cases.with_low_parts) and the packed item operand of the split route."""
	X = torch.from_numpy(nf.with_low_parts(case.X, seed)).cuda()
	Et = torch.from_numpy(np.ascontiguousarray(nf.with_low_parts(case.E, seed + 1).T)).cuda()
	return X, Et, ops.pack_split_bf16(Et, 1, row_multiple=32)


@pytest.mark.parametrize("name", ["nan-items", "nan-queries", "few-left"])
def test_split_route_equals_the_dense_route_on_nan_operands(ops, name):
	"""The same fp32 operands (NaN plants, low parts m 2^-12) through ops.score_topk_split and ops.score_topk_dense: ids and value bits."""
	case = _dense_case(ops, name)
	X, Et, Etp = _split_operands(ops, case, 11)
	want = ops.score_topk_dense(X, Et, case.k)
	got = ops.score_topk_split(X, Et, Etp, case.I, case.k)
	torch.cuda.synchronize()
	wv, wi = want.values.cpu().numpy(), want.indices.cpu().numpy()
	_, _, n_valid = nf.reference_topk(case.S, case.k)        # (NaN cells are where the integer operands have them: the low parts add none)
	assert ((wi >= 0).sum(1) == np.minimum(n_valid, case.k)).all() and not np.isnan(wv).any()
	assert np.array_equal(got.indices.cpu().numpy(), wi) and np.array_equal(got.values.cpu().numpy().view(np.uint32), wv.view(np.uint32))


def test_split_route_loses_items_with_an_infinite_entry(ops):
	"""The limit include/anncur_hip.h states for the split route: an operand entry of +-inf has no low part, and its score inside the sweep is
	lo_x (+-inf) + hi_x 0 + hi_x (+-inf).  Here column c0 of X is exactly representable in bf16 (lo_x = 0: 0 . inf = NaN) or has a low part of
	the opposite sign (inf - inf = NaN), so every item of J is a NaN in the sweep for every query and is never retrieved -- where the dense fp32
	route reports +inf for the queries with a positive entry.  Asserted exactly: the split route returns what the dense route returns when the
	items of J are NaN (inf-column, |J| = 3)."""
	case = _dense_case(ops, "inf-column-3")
	J, c0 = case.notes["J"], 1
	X, Et, _ = _split_operands(ops, case, 21)
	q = torch.arange(case.Q)
	X[:, c0] = torch.tensor([2.0, 0.0, -1.0])[q % 3].cuda()          # lo_x = 0
	X[q % 6 == 0, c0] = 2.0 - 2.0 ** -12                             # hi_x = 2, lo_x = -2^-12: the opposite sign
	assert torch.equal(Et[J, c0].cpu(), torch.full((3,), INF))
	Etp = ops.pack_split_bf16(Et, 1, row_multiple=32)
	dense = ops.score_topk_dense(X, Et, case.k)
	up = (q % 3 == 0).numpy()
	assert (dense.indices.cpu().numpy()[up, :3] == J[None, :]).all() and (dense.values.cpu().numpy()[up, :3] == INF).all()   # the dense route does return them
	Et_nan = Et.clone()
	Et_nan[J, c0] = NAN
	want = ops.score_topk_dense(X, Et_nan, case.k)
	got = ops.score_topk_split(X, Et, Etp, case.I, case.k)
	torch.cuda.synchronize()
	gi = got.indices.cpu().numpy()
	assert not np.isin(gi, J).any()
	assert np.array_equal(gi, want.indices.cpu().numpy()) and np.array_equal(got.values.cpu().numpy().view(np.uint32), want.values.cpu().numpy().view(np.uint32))
