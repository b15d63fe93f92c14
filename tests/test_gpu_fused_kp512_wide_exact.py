"""Exact-data tests of the fused score + top-k at Kp = 512 and on the wide kernel (Kp > 512): the three sweep bodies that had none --
  "q16"  scoreq16_kernel (csrc/score_q16.hpp): Kp = 512, the default; wave-level queue, XCD-sliced tickets, owner-map repair;
  "ring" score_sweep_kernel<512> (csrc/score32.hpp, the per-lane-ring body, mfma32=True): static interleaved tile shares;
  "wide" wide_kernel (csrc/score_wide.hpp): Kp = 640 and 1152, 256-item block tiles, static contiguous shares.
Every operand is a small integer, so every score is exact in fp32 in any order and the result must be THE top-k (values descending,
ties by ascending row) bit for bit.  Every call runs on a private workspace filled with 0xff (the q16 / ring chains rely on
zero_ws_header, launch_wide on a hipMemsetAsync of the header), against references built on the host (tests/fused_exact_cases.py), and
every test asserts the plan it means to run (ops.fused_plan) before it launches.

The select repairs overflowed segments and rescans a query that ends with fewer than k candidates, so a sweep that drops survivors can
still return THE top-k.  _check_sweep therefore also reads back what the sweep itself left in the workspace:
  - the prepass' group maxima (ops.fused_group_maxima), bit for bit against the host scores of the sampled tiles in the layout the prepass
    kernels write; tau0[q] = the k-th largest of them <= the true k-th score;
  - no fallback where none is legitimate: when no query has more than `segment_capacity` items at or above its threshold, no segment can
    overflow whatever the tile schedule, and every query collects >= k candidates, so nfb must be 0 (a lost carry, a stale ticket counter or a
    dropped survivor shows as a rescan);
  - the survivor count (ops.fused_survivors: the sum of the segment counts).  Read from the kernels: all three bodies count every OFFER --
    an item below I whose score is >= the lane's threshold --, also those beyond a segment's capacity (wq_drain's ds_add_rtn, flush_queue's and
    wide_kernel's ncand++); only the ring body can poison a count (a wrapped ring), which the select then repairs (nfb > 0).  So for one sweep
    stage the sum equals sum_q #{i < I : S[q, i] >= tau[q]} exactly (ring body: when nfb == 0), tau = tau0 cut to its 16-bit key prefix by the
    coarse threshold kernel (<= 4096 group maxima per query; exact above); for a staged plan it lies between sum_q #{S >= true k-th} and that sum.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_exact_cases as fx  # noqa: E402

pytestmark = pytest.mark.gpu
# Deterministic by default (the same examples every run); ANNCUR_FUZZ=1 draws fresh ones and ANNCUR_FUZZ_EXAMPLES=n draws more.
_FUZZ = os.environ.get("ANNCUR_FUZZ", "") not in ("", "0")
_N = int(os.environ.get("ANNCUR_FUZZ_EXAMPLES", "0"))

# body -> (Kp, the logical K of its cases unless a case names one, flags, "lg" of its plan, "stage_pred" of every stage -- None where the
# launcher ignores the word)
_BODY = {
	"q16": (512, 400, {}, 1, 4),
	"ring": (512, 257, {"mfma32": True}, 2, None),
	"wide": (640, 513, {}, 4, None),
	"wide1152": (1152, 1100, {}, 4, None),
}


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _plan(ops, body, Q, I, k, group, splits, capg, stage_end=None, leading=False):
	"""The plan of the case, asserted: body (lg, QT, stage_pred), prepass group, stages, item splits, segment capacity.  The expected words are
	those of a 256-CU device (an MI355X; the host query assumes the same)."""
	Kp, _, flags, lg, pred = _BODY[body]
	kw = dict(flags, leading_sample=leading)
	plan = ops.fused_plan(Q, I, Kp, k, **kw)
	stage_end = [-(-I // (256 if lg == 4 else 32))] if stage_end is None else stage_end
	assert plan["lg"] == lg and plan["QT"] == (2 if lg == 4 else 1) and not plan["ladder"], plan
	assert pred is None or plan["stage_pred"] == [pred] * len(stage_end), plan
	assert plan["group"] == group and plan["n_stages"] == len(stage_end) and plan["stage_end"] == stage_end, plan
	assert plan["splits"] == splits and plan["segment_capacity"] == capg, plan
	return plan, kw


def _check_sweep(ops, ws, S, plan, Kp, Q, I, k, kw, nfb, kth):
	"""What the sweep left in the workspace against the host scores (see the module docstring).  Returns (the no-fallback premise held,
	items at or above the threshold per query)."""
	lg = plan["lg"]
	gmax, info = ops.fused_group_maxima(ws, Q, I, Kp, k, **kw)
	want = fx.reference_gmax(S, fx.sample_tiles(plan, I, kw["leading_sample"], lg == 4), plan["group"])
	got = gmax.cpu()
	assert not info["prepass16"] and got.shape == want.shape == (Q, info["n_groups"]), (info, got.shape, want.shape)
	bad = (fx.bits(got) != fx.bits(want)).nonzero()
	assert bad.numel() == 0, f"{bad.shape[0]} group maxima differ; first (query, group) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
	tau0 = torch.topk(want, k, dim=1).values[:, -1].numpy()
	assert (tau0 <= kth).all(), "tau0 above the true k-th score"
	tau = fx.coarse_floor(tau0) if info["n_groups"] <= 4096 else tau0
	assert (tau <= tau0).all() and (tau > tau0 - np.maximum(1.0, np.abs(tau0) / 128)).all()   # (less than one bf16 ulp below)
	cnt = fx.count_ge(S, tau)
	premise = bool(cnt.max() <= plan["segment_capacity"])
	if premise:
		assert nfb == 0, f"{nfb} queries fell back although no query has more than {plan['segment_capacity']} items at or above its threshold"
	surv = ops.fused_survivors(ws, Q, I, Kp, k, **kw) * Q
	assert abs(surv - round(surv)) < 1e-3
	surv = int(round(surv))
	if lg != 2 or nfb == 0:
		if plan["n_stages"] == 1:
			assert surv == int(cnt.sum()), f"the sweep offered {surv} candidates, {int(cnt.sum())} items score at or above the thresholds"
		else:
			lo = int(fx.count_ge(S, kth).sum())
			assert lo <= surv <= int(cnt.sum()), f"staged sweep: {surv} candidates outside [{lo}, {int(cnt.sum())}]"
	return premise, cnt


def _run(ops, Kp, X, E_ik, S, k, plan, kw, perm=None, ldx_pad=0, calls=1):
	"""One case: poisoned workspace, the call (calls=2: twice on the same workspace, equal results), THE top-k, the sweep checks.
	E_ik [I x K].  Returns (nfb, the no-fallback premise held, items at or above the threshold per query, reference rows)."""
	Q, I = S.shape
	assert X.shape[1] == E_ik.shape[1] <= Kp and E_ik.shape[0] == I and int(S.abs().max()) < 1 << 24
	Xp, Etp = fx.device_operands(ops, X, E_ik, Kp, ldx_pad)
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	ids = perm.int().cuda() if perm is not None else None
	runs = []
	for _ in range(calls):
		(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws, item_ids=ids, **kw)
		torch.cuda.synchronize()
		runs.append((v.cpu(), i.cpu().long(), int(nfb.item())))
	v, got_i, nfb = runs[-1]
	for r in runs[:-1]:
		assert torch.equal(r[0], v) and torch.equal(r[1], got_i) and r[2] == nfb, "a second call on the same workspace gave another result"
	want_v, want_rows = fx.reference_topk(S, k)
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.double(), want_v.double())
	assert torch.equal(got_i, perm.long()[want_rows] if perm is not None else want_rows)
	premise, cnt = _check_sweep(ops, ws, S, plan, Kp, Q, I, k, kw, nfb, want_v[:, -1].numpy().astype(np.float64))
	return nfb, premise, cnt, want_rows


# ------------------------------------------------------------------ 1. ragged tail, all-negative scores
_RAGGED = [(b, 8192, t, K, s, c) for b, s, c in (("q16", 29, 128), ("ring", 129, 64)) for t, K in ((1, 257), (17, 400), (31, 512))]
_RAGGED += [("wide", 4096, t, 513, 9, 64) for t in (1, 31, 33, 255)]


@pytest.mark.parametrize("body,I0,tail,K,splits,capg", _RAGGED, ids=[f"{c[0]}-tail{c[2]}" for c in _RAGGED])
def test_all_negative_scores_with_a_ragged_tail(ops, body, I0, tail, K, splits, capg):
	"""Every real item scores in [-8, -1]; the zero rows that pad Et score 0 and would beat all of them (a sampled one would put tau0 at 0,
	above the true k-th score; a counted one shows in the survivor count).  Kp = 512: the smallest supported I plus a tail inside the last
	32-item tile.  Wide: a block tile holds 256 items and Et is padded to 32 rows only, so the tail tile is partly unbacked (its rows past Et
	re-read Et's last row)."""
	Q, k, I = 130, 100, I0 + tail
	plan, kw = _plan(ops, body, Q, I, k, group=4, splits=splits, capg=capg)
	X, E, S = fx.sparse_case(Q, I, K, seed=100 * tail + len(body), lo=-8, hi=-1, nnz=1, cmax=1)
	assert int(S.max()) == -1 and int(S.min()) == -8
	_run(ops, _BODY[body][0], X, E.t(), S, k, plan, kw)


# ------------------------------------------------------------------ 2. every k class x both group sizes, one stage
_ONE_STAGE = [   # body, Q, I, k, K (None: the body's), group, splits, segment capacity
	("q16", 1, 8203, 1, 257, 4, 29, 64),
	("q16", 1, 12005, 129, 257, 4, 32, 256),
	("q16", 1, 40001, 513, None, 4, 32, 512),            # (k > 512: the largest selector class)
	("q16", 130, 70031, 100, None, 16, 32, 256),
	("q16", 130, 70031, 129, 512, 16, 32, 256),
	("q16", 1, 131072 + 17, 2048, 257, 4, 241, 256),     # the smallest I the plan takes at k = 2048, plus a tail; 241 splits: the workgroup-level select
	("ring", 130, 70031, 129, None, 16, 244, 64),
	("ring", 1, 40001, 513, 400, 4, 251, 64),
	("ring", 1, 131072 + 17, 2048, None, 4, 241, 128),
	("wide", 1, 8203, 129, None, 4, 11, 128),
	("wide", 1, 24593, 513, None, 4, 14, 256),
	("wide", 1, 65567, 1, None, 16, 16, 64),
	("wide", 130, 70031, 129, None, 16, 16, 128),
	("wide", 1, 65536 + 17, 2048, None, 4, 52, 256),     # the smallest I at k = 2048, plus a tail
	("wide1152", 130, 20001, 100, None, 4, 16, 128),
]


@pytest.mark.parametrize("body,Q,I,k,K,group,splits,capg", _ONE_STAGE, ids=[f"{c[0]}-Q{c[1]}-I{c[2]}-k{c[3]}" for c in _ONE_STAGE])
def test_dense_operands_every_k_class_one_stage(ops, body, Q, I, k, K, group, splits, capg):
	"""Dense operands (X in [0, 2], E in [-2, 2] over all K columns: every k-step of the MFMA chains carries data) through the selector
	classes (k <= 128, <= 512, <= 1024 wave-level; 2048 workgroup-level) and both prepass group sizes, one sweep stage."""
	Kp, K0 = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=group, splits=splits, capg=capg)
	X, E, S = fx.dense_case(Q, I, K or K0, seed=I + k)
	_run(ops, Kp, X, E, S, k, plan, kw)


# ------------------------------------------------------------------ 3. staged sweeps
def _plant_over_stages(plan, I, k, wide):
	"""plant(E, g) for fx.sparse_case: k // 2 items inside the first stage's tiles and the rest behind it get the column 8 (the largest score
	of every query), k of them on the first row of k distinct sampled groups -- so tau0 is that score for every query and few items pass it --,
	the others (where the first stage holds fewer than k // 2 sampled groups) in unsampled tiles of the first stage."""
	first_end = min(plan["stage_end"][0] * (256 if wide else 32), I)
	tiles = fx.sample_tiles(plan, I, False, wide)
	reps = fx.group_representatives(tiles, plan["group"])

	def plant(E, g):
		r = reps[torch.randperm(reps.size, generator=g).numpy()]
		r1, r2 = r[r < first_end], r[r >= first_end]
		n1 = min(k // 2, r1.size)
		free = np.setdiff1d(np.arange(first_end // 32), tiles)
		extra = free[torch.randperm(free.size, generator=g).numpy()[:k // 2 - n1]] * 32 + 1
		assert n1 + extra.size == k // 2 and r2.size >= k - n1
		E[:, torch.from_numpy(np.concatenate([r1[:n1], extra, r2[:k - n1]]))] = 8
	return plant, first_end


_STAGED = [   # body, Q, I, k, stage ends, splits, segment capacity
	("q16", 513, 50007, 128, [281, 1563], 32, 1024),
	("q16", 385, 65567, 129, [221, 2049], 32, 1024),
	("q16", 1500, 200003, 512, [750, 2188, 6251], 32, 4096),
	("ring", 3000, 16391, 128, [180, 513], 21, 256),
	("wide", 513, 50007, 128, [35, 196], 16, 512),
	("wide", 385, 65567, 129, [28, 257], 16, 512),
	("wide", 1500, 200003, 512, [94, 274, 782], 16, 2048),
]


@pytest.mark.parametrize("body,Q,I,k,stage_end,splits,capg", _STAGED, ids=[f"{c[0]}-Q{c[1]}-I{c[2]}-k{c[3]}" for c in _STAGED])
def test_staged_sweep_carries_the_segment_counts(ops, body, Q, I, k, stage_end, splits, capg):
	"""Two and three sweep stages (`carry`: a later stage continues the segment counts of the one before; the thresholds are raised in
	between).  Sparse-X data; half of every query's top-k is planted inside the first stage's tiles and the rest behind it, on sampled
	groups, so that tau0 is the top score: no query has more than `segment_capacity` items at or above it, nothing may fall back, and a later
	stage that restarts its segments at 0 overwrites rows the reference names (the query then ends below k candidates: a rescan, nfb > 0)."""
	Kp, K = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=4, splits=splits, capg=capg, stage_end=stage_end)
	plant, first_end = _plant_over_stages(plan, I, k, plan["lg"] == 4)
	X, E, S = fx.sparse_case(Q, I, K, seed=I + k, plant=plant)
	assert int(S.abs().max()) <= 48
	nfb, premise, cnt, want_rows = _run(ops, Kp, X, E.t(), S, k, plan, kw)
	in_first = (want_rows < first_end).sum(1)
	assert (in_first >= k // 2).all() and (k - in_first >= k // 4).all(), "the planted halves are not in the reference top-k"
	assert premise and nfb == 0, (int(cnt.max()), capg, nfb)


# ------------------------------------------------------------------ 4. ties and flat rows
@pytest.mark.parametrize("const", [False, True], ids=["ties", "const"])
@pytest.mark.parametrize("body,splits,capg", [("q16", 32, 256), ("ring", 169, 64), ("wide", 16, 128)])
def test_ties_and_flat_rows(ops, body, splits, capg, const):
	"""Operands in [0, 1] x [-1, 1]: scores in a narrow band, thousands of items on every value -- and one constant score per query (every
	item passes the threshold, every segment overflows, the repair returns rows 0..k-1).  Q = 257: a partial row block in every body.
	The tie order must be exact."""
	Q, I, k = 257, 70031, 100
	Kp, K = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=16, splits=splits, capg=capg)
	X, E, S = fx.dense_case(Q, I, K, seed=7 + const, xmax=2 if const else 1, emax=1, const=const)
	nfb, _, cnt, want_rows = _run(ops, Kp, X, E, S, k, plan, kw)
	if const:
		assert (cnt == I).all() and nfb == Q and torch.equal(want_rows, torch.arange(k).expand(Q, k))
	else:
		assert (S.max(1).values - S.min(1).values).max() < 200 and cnt.min() > 4 * k   # (many more items at or above the threshold than values: ties)


# ------------------------------------------------------------------ 5. the index builder's hints
@pytest.mark.parametrize("body,splits,capg", [("q16", 32, 256), ("ring", 244, 64), ("wide", 16, 128)])
def test_leading_sample_and_item_ids(ops, body, splits, capg):
	"""leading_sample=True (the prepass samples the leading tiles; the ring body drains every tile of the first quarter) with item_ids a random
	permutation: ties are then ordered by row, as the header says, and the ids are item_ids[row].  The leading eighth of the items scores
	twice as wide as the rest, as norm-ordered rows would."""
	Q, I, k = 130, 70031, 100
	Kp, K = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=16, splits=splits, capg=capg, leading=True)
	g = torch.Generator().manual_seed(5)
	X, E, _ = fx.dense_case(Q, I, K, seed=11, xmax=1, emax=1)
	E[:I // 8] *= 2
	S = (X @ E.t()).to(torch.int32)
	_run(ops, Kp, X, E, S, k, plan, kw, perm=torch.randperm(I, generator=g))


# ------------------------------------------------------------------ 6. overflow and repair
@pytest.mark.parametrize("body,splits,capg", [("q16", 32, 256), ("ring", 244, 64), ("wide", 16, 128)])
def test_hot_items_overflow_every_schedule_and_are_repaired(ops, body, splits, capg):
	"""Every item of the unsampled tiles in the middle 80 % of the rows scores 7 or 8 times the query's coefficient sum, far above the
	sample's threshold: more survivors per query than ALL its segments hold together, so some segment overflows under any tile schedule.
	q16: owner-map repair under tickets; ring: interleaved static shares; wide: contiguous static shares.  nfb > 0, THE top-k (ties among
	the hot items by row), and the same again from a second call on the same workspace."""
	Q, I, k = 130, 70031, 100
	Kp, K = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=16, splits=splits, capg=capg)
	sampled = fx.sample_tiles(plan, I, False, plan["lg"] == 4)

	def plant(E, g):
		t = np.setdiff1d(np.arange(I // 10 // 32, 9 * I // 10 // 32), sampled)
		hot = torch.from_numpy((t[:, None] * 32 + np.arange(32)[None, :]).reshape(-1))
		E[:, hot] = torch.randint(7, 9, (hot.numel(),), generator=g, dtype=torch.int8)[None, :]
	X, E, S = fx.sparse_case(Q, I, K, seed=13, plant=plant)
	nfb, premise, cnt, _ = _run(ops, Kp, X, E.t(), S, k, plan, kw, calls=2)
	assert cnt.min() > plan["lg"] * splits * capg, (int(cnt.min()), plan)   # the premise: pigeonhole over the query's lg x splits segments
	assert not premise and nfb == Q


# ------------------------------------------------------------------ 7. padded query rows, partial row blocks
@pytest.mark.parametrize("Q", [1, 127, 129])
@pytest.mark.parametrize("body,splits,capg", [("q16", 29, 128), ("ring", 129, 64), ("wide", 11, 128)])
def test_strided_query_rows_and_partial_row_blocks(ops, body, splits, capg, Q):
	"""ldx = Kp + 16 with poison between the query rows (a kernel that assumed packed rows reads it as operand), Q one short of and one past
	the 128-query row block of the Kp = 512 bodies (the wide kernel's is 256: its lanes past Q re-read the block's last query)."""
	I, k = 8203, 100
	Kp, K = _BODY[body][:2]
	plan, kw = _plan(ops, body, Q, I, k, group=4, splits=splits, capg=capg)
	X, E, S = fx.dense_case(Q, I, K, seed=Q)
	_run(ops, Kp, X, E, S, k, plan, kw, ldx_pad=16)


# ------------------------------------------------------------------ fuzz
def test_exact_integer_fuzz_kp512_and_wide(ops):
	"""Small-integer operands over 257 <= K <= 1200 (Kp = 512 both bodies; 640 .. 1280 wide), with and without the hints.  Every draw is
	clamped to a supported shape (k is halved until the plan takes it; k = 1 is supported from I = 8203 on), and the test ends by asserting
	that no example was skipped."""
	seen = {"ran": 0, "skipped": 0}

	@settings(max_examples=_N or 12, deadline=None, derandomize=not _FUZZ, database=None)
	@given(Q=st.integers(1, 300), I=st.integers(8203, 60000), K=st.integers(257, 1200), kfrac=st.floats(0.0, 1.0), ring=st.booleans(), hints=st.booleans(),
		   kind=st.sampled_from(["ties", "const", "hot"]), seed=st.integers(0, 10 ** 6))
	def example(Q, I, K, kfrac, ring, hints, kind, seed):
		Q = max(1, min(Q, 6_000_000 // I))           # (bounded host work for the reference)
		Kp = ops.padded_k(K)
		k = 1 + int(kfrac * 599)
		while k > 1 and not ops.fused_supported(Q, I, Kp, k):
			k //= 2
		if not ops.fused_supported(Q, I, Kp, k):
			seen["skipped"] += 1
			return
		kw = dict(mfma32=ring and Kp == 512, leading_sample=hints)
		plan = ops.fused_plan(Q, I, Kp, k, **kw)
		assert plan["lg"] == (4 if Kp > 512 else 2 if ring else 1) and not plan["ladder"], plan
		g = torch.Generator().manual_seed(seed)
		X, E, S = fx.dense_case(Q, I, K, seed, xmax=1, emax=1, const=kind == "const")
		if kind == "hot":
			t = int(torch.randint(0, I // 64, (1,), generator=g))
			E[t * 32:(t + I // 1024) * 32] += 2
			S = (X @ E.t()).to(torch.int32)
		_run(ops, Kp, X, E, S, k, plan, kw, perm=torch.randperm(I, generator=g) if hints else None)
		seen["ran"] += 1

	example()
	assert seen["skipped"] == 0 and seen["ran"] > 0, seen
