"""Exact-data tests of the approximation-error sums err_sq[q] = sum_i (S_hat[q,i] - A[q,i])^2 and norm_sq[q] = sum_i A[q,i]^2 on every route:
evalf_kernel (ops.eval_fused), error_lds_kernel and error_kernel<float / bf16> (ops.approx_error_packed), gemm_kernel<.., 1> (the last I % 32
columns of those, and all of ops.approx_error), against an int64 reference on the CPU -- never route against route, no tolerance anywhere.

The data.  X [Q x K] has four +-1 per row (always column 0 and column K - 1, the other two walk over the 16-wide k-steps), E [K x I] holds
integers in [-e, e], so S_hat = X.E is an integer of magnitude <= 4 e.  A = S_hat + delta, delta an integer in [-d, d], zero for about half
the elements.  Everything is exact in bf16, every product and every partial sum is an integer below 2^24: the fp32 result is THE answer,
whatever the order of MFMAs, fmafs, shuffles and atomics.  Every case asserts that precondition on the host before it calls the GPU.

The poison.  A is the view [r0 : r0 + Q, c0 : c0 + I] of ONE larger buffer filled with NaN (guard rows before and after -- the kernels clamp
the rows past Q to the last row or to row 0 and drop their sums --, NaN in the pitch pad); Xp has ldx = Kp + 16 with NaN between the rows; Etp has NaN
rows past ceil32(I) (the rows I .. ceil32(I) - 1 are zero: the operand contract).  ops.eval_fused runs on the shared grow-only workspace filled
with 0xff.  A value read from outside the operands makes a sum NaN; a term lost, doubled or taken from a stale buffer changes an integer.

Mutations tried when this file was written, each built into a library of its own and loaded through ANNCUR_LIB, each run once on an MI355X
(118 tests then, 19 s; the rest of the GPU suite: see the commit).  "six" = the tolerance tests that covered these kernels before
(test_eval_fused_equals_the_two_kernel_route, test_eval_fused_random, test_approx_error_packed_matches_strided_and_fp64, test_approx_error_packed_random,
test_approx_error, test_error_kernels_with_a_row_pitch_beyond_the_32_bit_tile_offsets: 21 cases).  None survives this file:
  1. evalf_kernel: a_end = min(j_end, n_full_tiles - 1) (the last full tile's terms lost): 33 tests fail (every eval_fused test: route matrix,
     planted element, stages, candidate path, large I, repeated calls, random shapes); six: 7 of 21 fail.
  2. anncur_eval_fused_ex / anncur_approx_error_packed, tail call with I - I_full - 1 columns (last column lost): 61 tests fail; six: 11 fail.
     The tail call starting at column I_full - 1 (one column counted twice): 55 tests fail; six: 10 fail.
  3. asw[t] = 0 (the reads ignore the DMA's chunk swizzle) in error_lds_kernel: 32 tests fail, err wrong in exactly three rows of four, nrm right in
     every row; six: 15 fail (they compare the two routes).  In evalf_kernel: 30 tests fail, the same pattern; six: 7 fail.
  4. error_kernel: rowp without + 4 * h: 38 tests fail (err and nrm, every row); six: 5 fail.
  5. launch_fused: the evalf_kernel launch of stage 0 issued twice: 33 tests fail; six: 7 fail.
  6. sumsq_kernel: lda replaced by n_cols: the 4 padded test_sumsq_on_integers cases fail (NaN from the pad); six: none (nothing tested sumsq before).
(Counts are without test_diff_sumsq_f64_on_integers, whose own Y = None expectation was wrong in that run and has been corrected since.)
Needs an MI355X."""
import functools
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

pytestmark = pytest.mark.gpu
# Deterministic by default (the same examples every run); ANNCUR_FUZZ=1 draws fresh ones and ANNCUR_FUZZ_EXAMPLES=n draws more.
_FUZZ = os.environ.get("ANNCUR_FUZZ", "") not in ("", "0")
_N = int(os.environ.get("ANNCUR_FUZZ_EXAMPLES", "0"))

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
LIMIT = 1 << 24
# (the plans are sized from the card's compute-unit count: the shapes below were picked for the 256 CUs of an MI355X)
CU_NOTE = "plan assertion, not a kernel error: the shape no longer gives the plan this test was written for (another CU count or another plan_fused?)"


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _ceil32(n):
	return -(-n // 32) * 32


# ------------------------------------------------------------------ the data and the host reference
def _x_columns(Q, K):
	"""Four distinct columns per query: 0, K - 1, one at offset 1..14 of k-step q % (K // 16), one at the last (or first) column of k-step (7 q + 3) % (K // 16)."""
	q = torch.arange(Q, dtype=torch.int64)
	nk = max(K // 16, 1)
	c2 = 16 * (q % nk) + 1 + (q // nk * 3) % 14
	s3 = (7 * q + 3) % nk
	c3 = 16 * s3 + 15
	c3 = torch.where(c3 >= K - 1, 16 * s3, c3)
	cols = torch.stack([torch.zeros_like(q), torch.full_like(q, K - 1), c2, c3], 1)
	if K < 48:   # (tiny logical K: the walk cannot avoid the fixed columns; keep the two fixed ones and one in between)
		cols = torch.stack([torch.zeros_like(q), torch.full_like(q, K - 1), 1 + q % (K - 2)], 1)
	assert int(cols.max()) < K and all(cols[:, a].ne(cols[:, b]).all() for a in range(cols.shape[1]) for b in range(a)), "distinct columns"
	return cols


class Case:
	"""Host side of one problem: X, E (int8), S = X.E and A = S + delta (int16, CPU), err / nrm (int64) -- with the preconditions asserted."""

	def __init__(self, Q, I, K, e, d, seed, E=None, planted=False):
		g = np.random.default_rng(seed)
		self.Q, self.I, self.K = Q, I, K
		self.cols = _x_columns(Q, K)
		self.sign = torch.from_numpy(g.integers(0, 2, tuple(self.cols.shape)).astype(np.int8) * 2 - 1)
		self.E = torch.from_numpy(g.integers(-e, e + 1, (K, I), dtype=np.int8)) if E is None else E.to(torch.int8)
		self.A = torch.empty((Q, I), dtype=torch.int16)
		self.err = torch.empty(Q, dtype=torch.int64)
		self.nrm = torch.empty(Q, dtype=torch.int64)
		smax = 0
		for q0 in range(0, Q, 256):   # (row chunks bound the host memory of the large cells)
			q1 = min(Q, q0 + 256)
			S = torch.zeros((q1 - q0, I), dtype=torch.int16)
			for j in range(self.cols.shape[1]):
				S += self.E[self.cols[q0:q1, j]].to(torch.int16) * self.sign[q0:q1, j:j + 1].to(torch.int16)
			smax = max(smax, int(S.abs().max()))
			if planted:   # A = S_hat everywhere: the planted-element test moves one element on the device
				delta = torch.zeros_like(S)
			else:         # u in [0, 2 (2 d + 1)): the lower half maps to [-d, d], the upper half to 0 -- about half the elements are exact
				u = torch.from_numpy(g.integers(0, 2 * (2 * d + 1), (q1 - q0, I), dtype=np.int8)).to(torch.int16)
				delta = torch.where(u <= 2 * d, u - d, torch.zeros_like(u))
			self.A[q0:q1] = S + delta
			self.err[q0:q1] = (delta.to(torch.int32) ** 2).sum(1)
			self.nrm[q0:q1] = (self.A[q0:q1].to(torch.int32) ** 2).sum(1)
		# the preconditions of "bit for bit": bf16-exact operands, integer scores and sums below 2^24
		assert int(self.A.abs().max()) <= 256 and int(self.E.abs().max()) <= 256 and smax < LIMIT
		assert int(self.err.max()) < LIMIT and int(self.nrm.max()) < LIMIT, (int(self.err.max()), int(self.nrm.max()))

	def S(self):
		"""S_hat as int64 [Q x I] (small cells only: the top-k reference)."""
		S = torch.zeros((self.Q, self.I), dtype=torch.int64)
		for j in range(self.cols.shape[1]):
			S += self.E[self.cols[:, j]].to(torch.int64) * self.sign[:, j:j + 1].to(torch.int64)
		return S

	def X(self, Q=None):
		Q = self.Q if Q is None else Q
		X = torch.zeros((Q, self.K), dtype=torch.float32)
		X.scatter_(1, self.cols[:Q], self.sign[:Q].float())
		return X


@functools.lru_cache(maxsize=2)
def _cached_case(Q, I, K, e, d, seed):
	return Case(Q, I, K, e, d, seed)


# ------------------------------------------------------------------ the operands on the device, poisoned
def _xp(case, Kp, Q=None):
	"""Packed bf16 queries [Q x Kp] with ldx = Kp + 16 and NaN between the rows."""
	X = case.X(Q)
	buf = torch.full((X.shape[0], Kp + 16), NAN, dtype=BF16)
	buf[:, :Kp] = 0
	buf[:, :case.K] = X.to(BF16)
	assert torch.equal(buf[:, :case.K].float(), X)
	Xp = buf.cuda()[:, :Kp]
	assert Xp.stride(0) == Kp + 16
	return Xp


def _etp(case, Kp, E=None):
	"""Packed bf16 items [ceil32(I) + 64 x Kp]: rows I .. ceil32(I) - 1 zero (the contract), NaN in the 64 rows past them."""
	E = case.E if E is None else E
	I = E.shape[1]
	buf = torch.full((_ceil32(I) + 64, Kp), NAN, dtype=BF16)
	buf[:_ceil32(I)] = 0
	buf[:I, :case.K] = E.t().to(BF16)
	return buf.cuda()


def _guarded(A, dtype, pad, r0, c0, rows_after=3):
	"""The integer matrix A [Q x I] (CPU) as the view [r0 : r0 + Q, c0 : c0 + I] of one NaN-filled device buffer with row pitch
	32 + ceil8(I) + pad (c0 <= 32): guard rows before and after, NaN in front of column c0 and behind column I.  Asserts A.to(dtype) == A."""
	Q, I = A.shape
	assert 0 <= c0 <= 32
	pitch = 32 + -(-I // 8) * 8 + pad
	buf = torch.full((r0 + Q + rows_after, pitch), NAN, dtype=dtype, device="cuda")
	view = buf[r0:r0 + Q, c0:c0 + I]
	Ad = A.cuda()
	view.copy_(Ad)
	assert torch.equal(view.to(Ad.dtype), Ad), "the integer matrix is not exact in the operand's dtype"
	assert int(torch.isnan(buf).sum()) == buf.numel() - Q * I
	return view, buf


def _ws_state(ops):
	return sorted((key, buf.data_ptr(), buf.numel()) for key, buf in ops._Workspace._bufs.items())


def _poisoned(ops, call):
	"""call() on the shared workspace filled with 0xff over its whole size.  A call that had to grow it ran on fresh memory: it runs again."""
	for _ in range(3):
		for buf in ops._Workspace._bufs.values(): buf.fill_(0xff)
		before = _ws_state(ops)
		out = call()
		torch.cuda.synchronize()
		if _ws_state(ops) == before and before:
			return out
	raise AssertionError("the workspace keeps changing between identical calls")


def _equal_sums(got_err, got_nrm, case, what, Q=None):
	Q = case.Q if Q is None else Q
	ge, gn = got_err.cpu().double(), got_nrm.cpu().double()
	we, wn = case.err[:Q].double(), case.nrm[:Q].double()
	if torch.equal(ge, we) and torch.equal(gn, wn): return
	be, bn = (ge != we).nonzero()[:, 0], (gn != wn).nonzero()[:, 0]
	msg = f"{what}: err differs in {be.numel()} of {Q} rows, nrm in {bn.numel()}"
	if be.numel(): msg += f"; err rows {be[:8].tolist()} got {ge[be[:8]].tolist()} want {we[be[:8]].tolist()}"
	if bn.numel(): msg += f"; nrm rows {bn[:8].tolist()} got {gn[bn[:8]].tolist()} want {wn[bn[:8]].tolist()}"
	raise AssertionError(msg)


# routes: (name, dtype of A, pad of the pitch past ceil8(I))
EVALF, LDS, LANE16, LANE32, STRIDED32, STRIDED16 = "eval_fused", "packed_lds", "packed_lane_bf16", "packed_lane_fp32", "strided_fp32", "strided_bf16"
ROUTES = {EVALF: (BF16, 8), LDS: (BF16, 16), LANE16: (BF16, 4), LANE32: (F32, 4), STRIDED32: (F32, 3), STRIDED16: (BF16, 1)}


def _run_route(ops, route, case, Kp, Xp, Etp, A, k=10, hint=None, Q=None):
	"""One call of the route on the device operands -> (err, nrm, TopK or None); the route is asserted where Python can see it."""
	Q = case.Q if Q is None else Q
	I = case.I
	ld = ops._ld(A)
	if route == EVALF:
		assert ops.eval_fused_ok(Kp, A, Q, I, k), "the case left the one-pass route"
		assert A.dtype == BF16 and ld % 8 == 0 and ops.eval_fused_plan(Q, I, Kp, k)["stage_pred"][0] == 6
		top, err, nrm = _poisoned(ops, lambda: ops.eval_fused(Xp, Etp, A, I, k, hint=hint))
		return err, nrm, top
	if route in (LDS, LANE16, LANE32):
		assert ops.approx_error_packed_ok(Kp, A), "the case left the packed route"
		if route == LDS: assert A.dtype == BF16 and ld % 8 == 0 and 255 * ld * 2 + 64 < 1 << 32
		if route == LANE16: assert A.dtype == BF16 and ld % 8 == 4
		if route == LANE32: assert A.dtype == F32 and ld % 4 == 0
		err, nrm = ops.approx_error_packed(Xp, Etp, A, I)
		return err, nrm, None
	# the strided fp32-MFMA reduction on UNPACKED operands of the logical K (fp32 or bf16), any pitch
	dt = F32 if route == STRIDED32 else BF16
	if not hasattr(case, "_strided"): case._strided = {}
	if dt not in case._strided: case._strided[dt] = (case.X().to(dt).cuda(), case.E.t().to(dt).cuda())
	X, Et = case._strided[dt]
	err, nrm = ops.approx_error(X[:Q], Et, A)
	return err, nrm, None


def _a_for_route(route, A_cpu, r0=2, c0=None):
	dtype, pad = ROUTES[route]
	if c0 is None: c0 = {EVALF: 8, LDS: 16, LANE16: 8, LANE32: 4, STRIDED32: 1, STRIDED16: 3}[route]
	if route == LANE16 and r0 % 2: c0 += 4   # 16-byte aligned first element with a pitch of 4 mod 8: odd guard rows need c0 = 4 mod 8
	return _guarded(A_cpu, dtype, pad, r0, c0)


# ------------------------------------------------------------------ 1. the route matrix
Q_EDGES = [1, 127, 128, 129, 255, 256, 257, 600]
TAILS = [0, 1, 17, 31]


@pytest.mark.parametrize("Kp", [64, 128, 256, 512])
@pytest.mark.parametrize("tail", TAILS)
def test_route_matrix(ops, Kp, tail):
	"""Every route x Q in {1, 127 .. 257, 600} at I = 9216 + tail (288 full tiles; the tail goes to gemm_kernel<.., 1>), one data set per (Kp, tail),
	the smaller Q are row prefixes of it copied into their OWN guarded buffers (NaN right behind row Q - 1).  The strided route runs a logical
	K = Kp - 7 (not a multiple of 16) on fp32 and on bf16 operands.  A single row has no pitch -- ops passes lda = I -- so Q = 1 reaches the
	packed routes only where I itself is aligned (tail 0; never 4 mod 8: test_single_row_cells has the per-lane bf16 cell at Q = 1); the strided kernel takes the others."""
	I = 9216 + tail
	case = Case(600, I, Kp, 4, 3, seed=1000 * Kp + tail)
	caseK = Case(600, I, Kp - 7, 4, 3, seed=1000 * Kp + tail + 500)
	Etp = _etp(case, Kp)
	Adev, AdevK = case.A.cuda(), caseK.A.cuda()
	ran = {r: 0 for r in ROUTES}
	for Q in Q_EDGES:
		Xp = _xp(case, Kp, Q)
		for route in ROUTES:
			if route == EVALF and Kp > 256: continue
			c = caseK if route in (STRIDED32, STRIDED16) else case
			A, _ = _a_for_route(route, (AdevK if c is caseK else Adev)[:Q], r0=2 + Q % 2)
			if Q == 1 and route in (EVALF, LDS, LANE16, LANE32):
				if tail != 0 or route == LANE16: continue
			err, nrm, _ = _run_route(ops, route, c, Kp, Xp, Etp, A, Q=Q)
			_equal_sums(err, nrm, c, f"{route} Kp={Kp} Q={Q} I={I}", Q=Q)
			ran[route] += 1
	assert all(n >= 7 for r, n in ran.items() if not (r == EVALF and Kp > 256)), ran


@pytest.mark.parametrize("I", [1, 17, 31, 32, 33, 64, 95])
@pytest.mark.parametrize("Kp", [64, 512])
def test_few_items_tail_kernel_only_and_no_tail(ops, Kp, I):
	"""I < 32: the packed routes launch the tail kernel only; I = 32, 64: the tile kernel only; 33, 95: one or two tiles and a tail."""
	for Q in (1, 129, 257):
		case = Case(Q, I, Kp, 4, 3, seed=I + Q)
		caseK = Case(Q, I, Kp - 7, 4, 3, seed=I + Q + 1)
		Xp, Etp = _xp(case, Kp), _etp(case, Kp)
		for route in (LDS, LANE16, LANE32, STRIDED32, STRIDED16):
			if Q == 1 and route in (LDS, LANE16, LANE32): continue   # (lda = I for a single row: not a packed cell unless I is aligned)
			c = caseK if route in (STRIDED32, STRIDED16) else case
			A, _ = _a_for_route(route, c.A)
			err, nrm, _ = _run_route(ops, route, c, Kp, Xp, Etp, A)
			_equal_sums(err, nrm, c, f"{route} Kp={Kp} Q={Q} I={I}")


@pytest.mark.parametrize("Kp", [64, 128, 256, 512])
@pytest.mark.parametrize("I", [4, 36, 9216 + 4, 9216 + 8, 9216 + 12, 9216 + 16, 9216 + 20, 9216 + 24, 9216 + 28])
def test_single_row_cells(ops, Kp, I):
	"""Q = 1, where ops passes lda = I (a single row has no pitch) and every lane but one reads the clamp row.  I = 4 mod 8: the per-lane bf16 kernel
	(lda = 4 mod 8) and the per-lane fp32 one; I = 0 mod 8: the LDS kernel, eval_fused (Kp <= 256, enough items) and the per-lane fp32 kernel.
	The I % 32 columns behind the last full tile go to the tail kernel.  The row lies inside a NaN buffer with guard rows all the same."""
	case = Case(1, I, Kp, 4, 3, seed=I + Kp)
	Xp, Etp = _xp(case, Kp), _etp(case, Kp)
	routes = [LANE16, LANE32] if I % 8 == 4 else [LDS, LANE32] + ([EVALF] if Kp <= 256 and I > 9000 else [])
	for route in routes:
		A, _ = _a_for_route(route, case.A)
		assert ops._ld(A) == I
		err, nrm, _ = _run_route(ops, route, case, Kp, Xp, Etp, A)
		_equal_sums(err, nrm, case, f"{route} Kp={Kp} Q=1 I={I}")


# ------------------------------------------------------------------ 2. one planted element
def _split_edge_columns(plan, I):
	"""First and last column of every item split of every stage of an evalf plan (clipped to I)."""
	cols, begin = set(), 0
	for end, tps in zip(plan["stage_end"], plan["stage_tiles_per_split"]):
		for s in range(plan["splits"]):
			t0, t1 = begin + s * tps, min(begin + (s + 1) * tps, end)
			if t0 < t1: cols.update((32 * t0, min(32 * t1, I) - 1))
		begin = end
	assert begin == plan["n_tiles"]
	return cols


def _planted(ops, route, Kp, Q, I, k, positions_cols=None, rows=None):
	"""A = S_hat everywhere but ONE element, A[q*, i*] = S_hat + 1, moved on the device between calls: err must be exactly the unit vector
	e_{q*} and nrm the reference with that one square changed.  Sees a column summed by the tile kernel AND the tail kernel, a column of
	nobody, a permuted quad (the planted 1 stays but the rest of its row turns non-zero), a row taken from the clamp."""
	case = Case(Q, I, Kp, 4, 0, seed=7 * Kp + Q, planted=True)
	assert int(case.err.max()) == 0
	S = case.A   # (= S_hat)
	Xp, Etp = _xp(case, Kp), _etp(case, Kp)
	A, _ = _a_for_route(route, case.A)
	I_full = I // 32 * 32
	rows = [r for r in (0, 31, 32, 127, 128, 255, 256, Q - 1) if r < Q] if rows is None else rows
	cols = {0, 3, 4, 7, 8, 31, 32, I_full - 1, I_full, I - 1}
	if positions_cols is not None: cols |= positions_cols
	cols = sorted(c for c in cols if 0 <= c < I)
	nrm0 = case.nrm.double().cuda()
	zero = torch.zeros(Q, dtype=torch.float64, device="cuda")
	# baseline: nothing planted
	err, nrm, _ = _run_route(ops, route, case, Kp, Xp, Etp, A, k=k)
	assert torch.equal(err.double(), zero) and torch.equal(nrm.double(), nrm0), f"{route}: baseline (A = S_hat) not exact"
	n = 0
	for ci, c in enumerate(cols):
		# every (row, column) pair for the fixed columns; the split / tile edges (many) take one row each, rotating over the row list
		for q in (rows if c in (0, 3, 4, 7, 8, 31, 32, I_full - 1, I_full, I - 1) else [rows[ci % len(rows)]]):
			s = int(S[q, c])
			A[q, c] = s + 1
			if route == EVALF: top, err, nrm = ops.eval_fused(Xp, Etp, A, I, k)
			else: err, nrm, _ = _run_route(ops, route, case, Kp, Xp, Etp, A, k=k)
			want_e = zero.clone(); want_e[q] = 1
			want_n = nrm0.clone(); want_n[q] += 2 * s + 1
			ok = torch.equal(err.double(), want_e) and torch.equal(nrm.double(), want_n)
			A[q, c] = s
			if not ok:
				be = (err.double() != want_e).nonzero()[:, 0][:8].tolist()
				bn = (nrm.double() != want_n).nonzero()[:, 0][:8].tolist()
				raise AssertionError(f"{route} Kp={Kp}: planted A[{q}, {c}] (I_full {I_full}, I {I}): err rows {be} = {err[be].tolist()}, nrm rows {bn} = {(nrm[bn].double() - want_n[bn]).tolist()} off")
			n += 1
	return n


@pytest.mark.parametrize("Kp", [64, 128, 256])
def test_one_planted_element_eval_fused(ops, Kp):
	"""Rows {0, 31, 32, 127, 128, 255, 256, Q - 1} x the quad, tile and tail edges, and the first and last column of every item split."""
	Q, I, k = 300, 9216 + 17, 10
	plan = ops.eval_fused_plan(Q, I, Kp, k)
	assert plan["n_stages"] == 1 and plan["splits"] > 64, f"{CU_NOTE}: {plan}"
	assert _planted(ops, EVALF, Kp, Q, I, k, _split_edge_columns(plan, I)) > 80 + plan["splits"]


def test_one_planted_element_eval_fused_three_stages(ops):
	"""A three-stage plan: the first and last column of every item split of every stage (a tile summed by two stages, or by none, moves err)."""
	Q, I, Kp, k = 1793, 150017, 64, 500
	plan = ops.eval_fused_plan(Q, I, Kp, k)
	assert plan["n_stages"] == 3 and plan["splits"] >= 32, f"{CU_NOTE}: {plan}"
	edges = _split_edge_columns(plan, I)
	assert len(edges) > 4 * plan["splits"]
	_planted(ops, EVALF, Kp, Q, I, k, edges, rows=[0, 255, 256, 1535, 1536, 1791, 1792])


@pytest.mark.parametrize("route", [LDS, LANE16, LANE32])
@pytest.mark.parametrize("Kp", [64, 128, 256, 512])
def test_one_planted_element_packed(ops, route, Kp):
	"""The packed routes' item splits depend on the chip: the first and last column of EVERY tile covers them whatever they are."""
	Q, I = 300, 2048 + 17
	tiles = {32 * t for t in range(I // 32)} | {32 * t + 31 for t in range(I // 32)}
	assert _planted(ops, route, Kp, Q, I, 10, tiles) > 80 + 100


@pytest.mark.parametrize("route", [STRIDED32, STRIDED16])
def test_one_planted_element_strided(ops, route):
	"""gemm_kernel<.., 1> on its own: 128 x 128 tiles, logical K = 100."""
	assert _planted(ops, route, 100, 300, 700, 10, {127, 128, 255, 256, 383, 384, 639, 640}) > 80


# ------------------------------------------------------------------ 3. stages and splits of eval_fused
@pytest.mark.parametrize("Q,I,Kp,k,stages", [(130, 40000 + 17, 128, 100, 1), (6000, 12288 + 17, 64, 10, 1), (1793, 50017, 128, 100, 2), (1793, 150017, 64, 500, 3)])
def test_eval_fused_stages_and_splits(ops, Q, I, Kp, k, stages):
	"""1, 2 and 3 sweep stages; few queries (every tile share is a few tiles, hundreds of splits add into one row) and many queries (few splits,
	long shares: the exact-tile buffers are refilled two tiles ahead many times).  The plan is asserted, not guessed."""
	plan = ops.eval_fused_plan(Q, I, Kp, k)
	assert plan["n_stages"] == stages == len(plan["stage_end"]) and plan["stage_end"][-1] == plan["n_tiles"] == -(-I // 32), f"{CU_NOTE}: {plan}"
	assert all(p == 6 for p in plan["stage_pred"]) and plan["lg"] == 1, plan
	if Q == 130: assert plan["splits"] > 128, f"{CU_NOTE}: {plan}"
	if Q == 6000: assert plan["splits"] <= 32 and plan["stage_tiles_per_split"][0] >= 12, f"{CU_NOTE}: {plan}"
	case = Case(Q, I, Kp, 4, 3, 31)
	Xp, Etp = _xp(case, Kp), _etp(case, Kp)
	A, _ = _a_for_route(EVALF, case.A)
	err, nrm, top = _run_route(ops, EVALF, case, Kp, Xp, Etp, A, k=k)
	_equal_sums(err, nrm, case, f"eval_fused {stages} stage(s) Q={Q} I={I}")
	# the same cell again, on the workspace as the first call left it: nothing carried
	top2, err2, nrm2 = ops.eval_fused(Xp, Etp, A, I, k)
	_equal_sums(err2, nrm2, case, "eval_fused, second call on the same workspace")
	assert torch.equal(top.values, top2.values) and torch.equal(top.indices, top2.indices)


# ------------------------------------------------------------------ 4. the candidate path under load
def _topk_reference(S, k):
	"""THE top-k of integer scores S [Q x I] (int64, CPU): (values, rows), values descending, ties by ascending row."""
	I = S.shape[1]
	assert I < 1 << 27 and int(S.abs().max()) < LIMIT
	key = S * (1 << 27) - torch.arange(I, dtype=torch.int64)
	rows = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows), rows


@pytest.mark.parametrize("kind", ["const", "hot", "ties"])
@pytest.mark.parametrize("Kp,k", [(64, 10), (128, 100), (256, 300)])
def test_eval_fused_candidate_path_under_load(ops, kind, Kp, k):
	"""Cells where (nearly) every item passes the first threshold -- one constant score; a hot range of tiles far above the rest; ties
	everywhere -- so the wave queue drains in mid-tile, segments overflow and the select repairs.  The sums are exact all the same and the
	top-k is THE top-k (values descending, ties by ascending row), with and without the first-threshold hint (descending- and
	ascending-norm copies of the item rows): same bits."""
	Q, I = 300, 20000 + 17
	g = np.random.default_rng(Kp + k)
	if kind == "const":
		E = torch.zeros((Kp, I), dtype=torch.int8); E[0] = 1; E[Kp - 1] = 1
	elif kind == "hot":
		E = torch.from_numpy(g.integers(-1, 2, (Kp, I), dtype=np.int8))
		E[:, 32 * 200:32 * 330] += 3
	else:
		E = torch.from_numpy(g.integers(-1, 2, (Kp, I), dtype=np.int8))
	case = Case(Q, I, Kp, 4, 3, seed=Kp + k, E=E)
	S = case.S()
	Xp, Etp = _xp(case, Kp), _etp(case, Kp)
	A, _ = _a_for_route(EVALF, case.A)
	want_v, want_rows = _topk_reference(S, k)
	norms = (case.E.to(torch.int64) ** 2).sum(0)
	results = []
	for hint_kind in (None, "descending", "ascending"):
		hint = None
		if hint_kind is not None:
			order = torch.argsort(norms, descending=hint_kind == "descending", stable=True)
			hint = _etp(case, Kp, E=case.E[:, order])
			assert hint.shape == Etp.shape
		err, nrm, top = _run_route(ops, EVALF, case, Kp, Xp, Etp, A, k=k, hint=hint)
		_equal_sums(err, nrm, case, f"eval_fused {kind} hint={hint_kind}")
		gi = top.indices.cpu().long()
		assert ((gi >= 0) & (gi < I)).all()
		assert torch.equal(top.values.cpu().double(), want_v.double()), f"{kind} hint={hint_kind}: values"
		assert torch.equal(gi, want_rows), f"{kind} hint={hint_kind}: rows (ties by ascending row)"
		results.append(top)
	for t in results[1:]:
		assert torch.equal(t.values, results[0].values) and torch.equal(t.indices, results[0].indices)


# ------------------------------------------------------------------ 5. large I
@pytest.mark.parametrize("route", list(ROUTES))   # (varies fastest: the two host data sets of an item count are built once)
@pytest.mark.parametrize("I,e,d,Kp", [(262144 + 17, 4, 3, 256), (500000 + 17, 2, 2, 128)])
def test_large_item_counts(ops, route, I, e, d, Kp):
	"""Many tiles per split and long chains of atomics; Q = 130 (two rows in the second sub-tile of the first wave)."""
	Q = 130
	K = Kp - 7 if route in (STRIDED32, STRIDED16) else Kp
	case = _cached_case(Q, I, K, e, d, 5)
	Xp, Etp = (_xp(case, Kp), _etp(case, Kp)) if K == Kp else (None, None)
	A, _ = _a_for_route(route, case.A)
	err, nrm, _ = _run_route(ops, route, case, Kp, Xp, Etp, A)
	_equal_sums(err, nrm, case, f"{route} I={I}")


# ------------------------------------------------------------------ nothing carried between calls
def test_smaller_cell_after_a_larger_one_and_repeated_calls(ops):
	"""A large cell, then a smaller one on the workspace and allocator state the first left (nothing poisoned in between), then every entry point
	twice in a row on the same operands: each result equals the reference (the sums are zeroed by every call)."""
	Kp, k = 128, 10
	big = Case(600, 40000 + 31, Kp, 4, 3, seed=1)
	small = Case(129, 9216 + 1, Kp, 4, 3, seed=2)
	Ab, _ = _a_for_route(EVALF, big.A)
	err, nrm, _ = _run_route(ops, EVALF, big, Kp, _xp(big, Kp), _etp(big, Kp), Ab, k=k)
	_equal_sums(err, nrm, big, "the larger cell")
	state = _ws_state(ops)
	Xp, Etp = _xp(small, Kp), _etp(small, Kp)
	As, _ = _a_for_route(EVALF, small.A)
	top, err, nrm = ops.eval_fused(Xp, Etp, As, small.I, k)
	assert _ws_state(ops) == state, "the smaller cell was to reuse the larger one's workspace"
	_equal_sums(err, nrm, small, "the smaller cell after the larger one")
	for route in ROUTES:
		c = small if route not in (STRIDED32, STRIDED16) else Case(129, 9216 + 1, Kp - 7, 4, 3, seed=3)
		A, _ = _a_for_route(route, c.A)
		for turn in (1, 2):
			if route == EVALF: _, err, nrm = ops.eval_fused(Xp, Etp, A, c.I, k)
			else: err, nrm, _ = _run_route(ops, route, c, Kp, Xp, Etp, A)
			_equal_sums(err, nrm, c, f"{route}, call {turn} on the same operands")


# ------------------------------------------------------------------ 6. bounded sweep over shapes, pitches, offsets
def test_error_sums_random_shapes(ops):
	"""Hypothesis over Q, I, K, dtype, pad, r0, c0.  Each drawn cell runs on every route that takes it (asserted through the predicates) and always on
	the strided kernel, which takes any operands.  A draw that neither eval_fused nor a packed kernel took counts as skipped (it reached the strided
	kernel only): more than a quarter of them fails the test, and the tile kernels must have had their share of the draws."""
	seen = {"examples": 0, "skipped": 0, EVALF: 0, "packed": 0}

	@settings(max_examples=_N or 30, deadline=None, derandomize=not _FUZZ, database=None, suppress_health_check=list(HealthCheck))
	@given(aim=st.sampled_from([EVALF, EVALF, "packed", "any"]), Q=st.integers(1, 400), I=st.integers(1, 30000), Kp=st.sampled_from([64, 128, 256, 512]), kdrop=st.sampled_from([0, 0, 1, 9, 16]),
		   dtype=st.sampled_from([BF16, BF16, F32]), pad=st.sampled_from([0, 4, 8, 8, 12, 16, 40]), r0=st.integers(0, 3), c0=st.sampled_from([0, 4, 8, 8, 16, 24, 32]),
		   e=st.sampled_from([1, 4]), d=st.sampled_from([1, 3]), seed=st.integers(0, 10 ** 6))
	def run(aim, Q, I, Kp, kdrop, dtype, pad, r0, c0, e, d, seed):
		# the draw is steered into the domain of the route it aims at (the predicates still decide what runs): the one-pass route wants a bf16 matrix,
		# 16-byte aligned rows, Kp <= 256 and enough items for a sampled threshold; the packed routes a pitch of 0 mod 4 and an aligned first element
		if aim == EVALF: dtype, pad, c0, Kp, I, Q = BF16, pad // 8 * 8, c0 // 8 * 8, min(Kp, 256), 8192 + I % 21809, max(Q, 2)
		elif aim == "packed" and dtype == BF16: r0, c0, Q = r0 // 2 * 2, c0 // 8 * 8, max(Q, 2)
		Q = max(1, min(Q, 6_000_000 // I))
		K = Kp - kdrop
		case = Case(Q, I, K, e, d, seed)
		A, _ = _guarded(case.A, dtype, pad, r0, c0)
		Xp, Etp = _xp(case, Kp), _etp(case, Kp)
		seen["examples"] += 1
		k = min(10, I)
		if ops.eval_fused_ok(Kp, A, Q, I, k):
			top, err, nrm = _poisoned(ops, lambda: ops.eval_fused(Xp, Etp, A, I, k))
			_equal_sums(err, nrm, case, f"eval_fused Q={Q} I={I} Kp={Kp} pad={pad} r0={r0} c0={c0}")
			seen[EVALF] += 1
		if ops.approx_error_packed_ok(Kp, A):
			err, nrm = ops.approx_error_packed(Xp, Etp, A, I)
			_equal_sums(err, nrm, case, f"approx_error_packed Q={Q} I={I} Kp={Kp} {dtype} pad={pad} r0={r0} c0={c0}")
			seen["packed"] += 1
		else:
			assert Q == 1 or (ops._ld(A) % 4) or (A.data_ptr() % 16), "a cell the packed route should have taken"
			seen["skipped"] += 1   # (eval_fused's domain lies inside the packed routes': no tile kernel saw this draw)
		err, nrm = ops.approx_error(case.X().to(dtype).cuda(), case.E.t().to(dtype).cuda(), A)
		_equal_sums(err, nrm, case, f"approx_error Q={Q} I={I} K={K} {dtype} pad={pad} r0={r0} c0={c0}")

	run()
	assert seen["examples"] >= 10 and 4 * seen["skipped"] <= seen["examples"], seen
	assert seen[EVALF] >= seen["examples"] // 4 and seen["packed"] >= seen["examples"] // 2, seen


# ------------------------------------------------------------------ 7. the small kernels beside them
@pytest.mark.parametrize("rows,cols,pad", [(1, 1, 0), (1, 2047, 1), (1, 2048, 0), (1, 2049, 7), (37, 57, 3), (8, 256, 8), (1100, 2048, 5), (2049, 1031, 1), (0, 5, 0), (5, 0, 0), (0, 0, 0)])
def test_sumsq_on_integers(ops, rows, cols, pad):
	"""Integer fp32 matrix in [-2, 2] with NaN in the pitch pad: the sum of squares is exact; around one block's 256 x 8 elements and above
	1024 blocks (the grid-stride loop runs); an empty matrix sums to 0."""
	g = np.random.default_rng(rows * 31 + cols)
	M = torch.from_numpy(g.integers(-2, 3, (rows, cols)).astype(np.int64))
	want = int((M * M).sum())
	assert want < LIMIT
	buf = torch.full((rows + 1, cols + pad), NAN, dtype=F32, device="cuda")
	A = buf[:rows, :cols]
	A.copy_(M.float().cuda())
	out = torch.full((1,), NAN, dtype=F32, device="cuda")
	got = ops.sumsq(A, out=out)
	assert got.data_ptr() == out.data_ptr() and float(got.item()) == float(want), (float(got.item()), want)
	assert float(ops.sumsq(A).item()) == float(want)   # a fresh output, and a second call


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048, 2049, 1_000_003, 2_200_003])
def test_diff_sumsq_f64_on_integers(ops, n):
	"""[sum (X - Y)^2, sum X^2] on integer-valued fp64 (exact far below 2^53), Y given and Y = None ([0, sum X^2]); n past 1024 blocks x 2048 elements too."""
	g = np.random.default_rng(n)
	X = torch.from_numpy(g.integers(-1000, 1001, n))
	Y = torch.from_numpy(g.integers(-1000, 1001, n))
	Xd, Yd = X.double().cuda(), Y.double().cuda()
	out = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
	got = ops.diff_sumsq_f64(Xd, Yd, out=out).cpu()
	assert got.tolist() == [float(((X - Y) ** 2).sum()), float((X * X).sum())]
	got = ops.diff_sumsq_f64(Xd).cpu()
	assert got.tolist() == [0.0, float((X * X).sum())]   # no Y: no difference term (pinv.py reads [1] only)


@pytest.mark.parametrize("M,N", [(1, 1), (3, 5), (16, 16), (17, 15), (255, 3), (64, 300)])
@pytest.mark.parametrize("mode", ["plain", "src_t", "dst_t", "both_t"])
def test_scale_copy_exact(ops, M, N, mode):
	"""dst = alpha / divide_by[0] * src with alpha = 0.5 and a device scalar 4 (0.125: every product exact), transposed source and / or
	destination views of padded buffers; NaN around the destination view must survive and NaN around the source must not be read."""
	g = np.random.default_rng(M * 100 + N)
	V = torch.from_numpy(g.integers(-100, 101, (M, N)).astype(np.float32))
	def view(t):
		buf = torch.full((N + 2, M + 3) if t else (M + 2, N + 3), NAN, dtype=F32, device="cuda")
		return (buf[1:N + 1, 2:M + 2].t() if t else buf[1:M + 1, 2:N + 2]), buf
	src, _ = view(mode in ("src_t", "both_t"))
	dst, dbuf = view(mode in ("dst_t", "both_t"))
	src.copy_(V.cuda())
	inside = torch.zeros_like(dbuf, dtype=torch.bool)
	(inside[1:N + 1, 2:M + 2] if mode in ("dst_t", "both_t") else inside[1:M + 1, 2:N + 2]).fill_(True)
	div = torch.tensor([4.0], dtype=F32, device="cuda")
	out = ops.scale_copy(src, dst, alpha=0.5, divide_by=div)
	assert out.data_ptr() == dst.data_ptr()
	assert torch.equal(dst.cpu(), V * 0.125)
	assert torch.equal(torch.isnan(dbuf), ~inside), "NaN outside the destination view must survive, none inside"
	ops.scale_copy(src, dst, alpha=-2.0)   # no divisor
	assert torch.equal(dst.cpu(), V * -2.0) and torch.equal(torch.isnan(dbuf), ~inside)
