"""Exact-data stress of the fused score + top-k for Kp <= 256 (csrc/score16.hpp, planned by plan_fused in csrc/score_fused.hip).

Every score here is a small integer: the bf16 operands are exact and every fp32 sum is exact (|S| < 2^24), so the result must be THE
top-k -- values descending, ties by ascending row -- bit for bit.  Where the plan runs the threshold ladder, the ladder's own state
(ops.fused_ladder_state) is checked as well, because the select's repair / full rescan can hide a threshold that moved too far:
  (a) for every query and level j, the candidates counted at level >= j never outnumber the items that truly score >= levels[j - 1]
      (a phantom, carried or double count, whatever the timing);
  (b) tau0 <= tau_final <= the true k-th score;
  (c) the levels ascend and start at or above tau0.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_exact_cases as fx  # noqa: E402

pytestmark = pytest.mark.gpu
# Deterministic by default (the same examples every run); ANNCUR_FUZZ=1 draws fresh ones and ANNCUR_FUZZ_EXAMPLES=n draws more.
_FUZZ = os.environ.get("ANNCUR_FUZZ", "") not in ("", "0")
_N = int(os.environ.get("ANNCUR_FUZZ_EXAMPLES", "0"))


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _reference(S, k):
	"""THE top-k of integer scores S [Q x I] (int64, CPU): (values, rows), values descending, ties by ascending row."""
	I = S.shape[1]
	assert I < 1 << 27 and int(S.abs().max()) < 1 << 24
	key = S * (1 << 27) - torch.arange(I, dtype=torch.int64)   # one key per (score, row): larger score first, then smaller row
	rows = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows), rows


def _check_ladder(state, S, kth):
	"""Invariants (a)-(c) of the ladder state against the true integer scores S [Q x I] (or [1 x I]: the same row for every query) and the
	true k-th scores kth [Q]."""
	lv = state["levels"].astype(np.float64)
	cnt = state["counts"].astype(np.int64)
	tf, t0 = state["tau_final"].astype(np.float64), state["tau0"].astype(np.float64)
	kth = np.broadcast_to(np.asarray(kth, dtype=np.float64), t0.shape)
	assert (np.diff(lv, axis=1) >= 0).all() and (lv[:, 0] >= t0).all(), "(c) levels out of order or below tau0"
	counted_ge = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]   # [q, j - 1]: counted at level >= j
	if S.shape[0] == 1:
		srt = np.sort(S[0].numpy().astype(np.float64))
		true_ge = srt.size - np.searchsorted(srt, lv, side="left")
	else:
		Sd = S.double()
		true_ge = np.stack([(Sd >= torch.from_numpy(np.ascontiguousarray(lv[:, j]))[:, None]).sum(1).numpy() for j in range(lv.shape[1])], axis=1)
	over = np.argwhere(counted_ge > true_ge)
	assert over.size == 0, f"(a) query {over[0][0]}, level {over[0][1] + 1}: {counted_ge[tuple(over[0])]} counted >= {lv[tuple(over[0])]}, only {true_ge[tuple(over[0])]} items"
	assert (t0 <= tf).all(), "(b) tau_final below tau0"
	bad = np.nonzero(tf > kth)[0]
	assert bad.size == 0, f"(b) tau_final above the true k-th score: query {bad[0]}: {tf[bad[0]]} > {kth[bad[0]]}"


def _etp_from_first_column(ops, scores, Kp):
	"""Packed Et whose column 0 holds `scores` (int64 [I]) and nothing else: with X = e_0 the score of item i is scores[i]."""
	I = scores.shape[0]
	Etp = torch.zeros((-(-I // 32) * 32, Kp), dtype=torch.bfloat16, device="cuda")
	Etp[:I, 0] = torch.from_numpy(scores).to(torch.bfloat16).cuda()
	return Etp


# ------------------------------------------------------------------ counter flood
def _flood_scores(plan, I, k, b, leading):
	"""Scores that put the ladder at exactly 1..8 above tau0 = 0 and then flood the counter of level b.
	Sampled tiles: k - 1 groups with a maximum >= 2 (ladder_top_rank of them at 8, the rest 2..7), every other group's maximum 0 -- so the
	k-th largest group maximum is 0 and the ladder's top (rank ladder_top_rank) is 8.  Every other item scores b: > 2^17 items at one level."""
	n_full, n_st, k2 = I // 32, plan["n_sample_tiles"], plan["ladder_top_rank"]
	gpt = 2 if plan["group"] == 16 else 8   # group maxima per sampled tile: 2 groups of 16 items, or 8 of 4
	tiles = np.arange(n_st, dtype=np.int64) if leading else (np.arange(n_st, dtype=np.int64) * n_full) // n_st   # (the prepass' tile_of)
	s = np.full(I, b, dtype=np.int64)
	s[(tiles[:, None] * 32 + np.arange(32)[None, :]).ravel()] = 0
	# row 4 g of a sampled tile lies in group g: 4 items -> rows 4g..4g+3; 16 items -> rows with (row >> 2) & 1 == g (the prepass' epilogue)
	slots = (tiles[:, None] * 32 + 4 * np.arange(gpt)[None, :]).ravel()[:k - 1]
	assert slots.size == k - 1
	s[slots] = np.where(np.arange(k - 1) < k2, 8, 2 + np.arange(k - 1) % 6)
	assert (s == b).sum() >= 1 << 17
	return s


@pytest.mark.parametrize("leading", [True, False], ids=["leading", "strided"])
@pytest.mark.parametrize("k", [129, 500, 1000])
@pytest.mark.parametrize("Q", [1, 64, 256])
@pytest.mark.parametrize("b", range(1, 9))
def test_fused_ladder_counter_flood(ops, leading, k, Q, b):
	"""More than 2^17 items at ONE ladder level b (b odd: a low-half field, whose wrap would carry into level b + 1), k - 1 items above
	the bulk, I = 2^18 + 17 (a ragged tail).  The ladder must end exactly at level b (for b = 1 the true k-th item is the first bulk
	item: one level too far drops it), the counts must stay within the items that exist, and the result must be THE top-k.  Segment
	overflow and the select's repair are legitimate here (every bulk item passes tau0 = 0); the invariants see through them."""
	I, Kp = (1 << 18) + 17, 256
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=leading)
	assert plan["ladder"] and plan["lg"] == 1 and plan["n_stages"] == 1, plan
	s = _flood_scores(plan, I, k, b, leading)
	Xp = torch.zeros((Q, Kp), dtype=torch.bfloat16, device="cuda")
	Xp[:, 0] = 1
	Etp = _etp_from_first_column(ops, s, Kp)
	ws = ops.fused_workspace(Q, I, Kp, k, Xp.device)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, leading_sample=leading)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=leading)
	# precondition: the case builds the ladder it means to test (tau0 = 0, levels 1..8)
	assert (state["tau0"] == 0).all(), state["tau0"][:4]
	assert (state["levels"] == np.arange(1, 9, dtype=np.float32)[None, :]).all(), state["levels"][:2]
	S = torch.from_numpy(s)[None, :]
	want_v, want_rows = _reference(S, k)
	assert int(want_v[0, -1]) == b
	_check_ladder(state, S, float(b))
	if Q == 1:
		# one query: its wave's queue never reaches the mid-tile drain (which does not count for the ladder), every candidate is counted, and
		# the flood must move the threshold to level b -- the ladder is live, not merely harmless (many queries in a flood spill into that drain)
		assert (state["tau_final"] == b).all(), state["tau_final"]
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double().expand(Q, k))
	assert torch.equal(got_i, want_rows.expand(Q, k))


# ------------------------------------------------------------------ all-negative scores, ragged I
@pytest.mark.parametrize("body", ["ladder", "staged", "mfma32", "qt1"])
@pytest.mark.parametrize("tail", [1, 17, 31])
@pytest.mark.parametrize("k", [100, 700])
def test_fused_all_negative_scores_with_a_ragged_tail(ops, body, tail, k):
	"""Every real item scores in [-8, -1]; the zero rows that pad Et to whole tiles score 0 and would beat all of them.  They must never be
	returned, counted by the ladder or sampled by the prepass (tau0 would be 0, above the true k-th score)."""
	Q, K, I = 130, 128, 2200 * 32 + tail
	g = torch.Generator().manual_seed(1000 * tail + k)
	E = torch.randint(-8, 0, (K, I), generator=g)
	col = torch.randint(0, K, (Q,), generator=g)
	X = torch.zeros(Q, K)
	X[torch.arange(Q), col] = 1
	S = E[col]                                   # [Q x I]: query q reads row col[q] of E
	Kp = ops.padded_k(K)
	Xp = ops.pack_bf16(X.cuda(), Kp)
	Etp = ops.pack_bf16(E.t().float().contiguous().cuda(), Kp, row_multiple=32)
	assert Etp.shape[0] > I and not Etp[I:].any()
	kw = dict(staged=body == "staged", mfma32=body == "mfma32", qt1=body == "qt1")
	plan = ops.fused_plan(Q, I, Kp, k, **kw)
	assert plan["ladder"] == (body == "ladder"), plan
	assert plan["QT"] == (1 if body == "qt1" else 2) and (body == "staged" or plan["lg"] == (1 if body == "ladder" else 2)), plan
	ws = ops.fused_workspace(Q, I, Kp, k, Xp.device)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, **kw)
	want_v, want_rows = _reference(S, k)
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(got_i, want_rows)
	if plan["ladder"]:
		_check_ladder(ops.fused_ladder_state(ws, Q, I, Kp, k, **kw), S, want_v[:, -1].numpy())
	else:
		from anncur_amd import _lib
		with pytest.raises(_lib.AnncurHipError, match="no threshold ladder"):
			ops.fused_ladder_state(ws, Q, I, Kp, k, **kw)


# ------------------------------------------------------------------ qt1: one sub-tile per wave on the sweep's shared tile schedule
_QT1_Q, _QT1_I, _QT1_K, _QT1_SPLITS = 130, 33011, 100, 207
# split s sweeps the tiles s, s + 207, ...: 1032 tiles = 204 splits of five (the last tile ends in the first accumulator) and three of four.
# Hot tiles, every item of which is every query's best score: the first tile of a split, the last of a five-tile and of a four-tile split.
_QT1_HOT = (100, 10 + 4 * _QT1_SPLITS, 205 + 3 * _QT1_SPLITS)


@functools.lru_cache(maxsize=2)
def _qt1_case(K):
	def plant(E, g):
		for t in _QT1_HOT:
			E[:, t * 32:(t + 1) * 32] = 8
	X, E, S = fx.sparse_case(_QT1_Q, _QT1_I, K, seed=K, plant=plant)
	return X, E, S, fx.reference_topk(S, _QT1_K)


@pytest.mark.parametrize("leading", [False, True], ids=["strided", "leading"])
@pytest.mark.parametrize("Kp", [128, 256])
def test_fused_qt1_static_shares_of_both_parities(ops, Kp, leading):
	"""ANNCUR_TOPK_QT1 (score_sweep_kernel<Kp, false, 1>: stagger1_tile on the schedule it shares with the Kp = 512 ring body, static interleaved
	shares).  Q = 130: two row blocks, the second almost all padding; 1032 tiles over 207 splits, so workgroups end on either accumulator;
	a ragged tail of 19.  Three whole tiles score every query's maximum: each lane finds sixteen survivors in one tile, more than its ring
	holds, and hands the raw accumulator to the next step's drain (or, for a split's last tile, to the final one).  THE top-k bit for bit,
	no fallback (no segment overflows: checked on the host scores), and the sweep offers exactly the items at or above the thresholds.
	Mutation (a build of its own, on an MI355X): the step's drain given the previous tile's first item for a raw ring instead of the
	one before it -- all four cases fail on the ids."""
	Q, I, k = _QT1_Q, _QT1_I, _QT1_K
	kw = dict(qt1=True, leading_sample=leading)
	plan = ops.fused_plan(Q, I, Kp, k, **kw)
	assert plan["QT"] == 1 and plan["lg"] == 2 and not plan["ladder"] and plan["n_stages"] == 1, plan
	S_, n_tiles = plan["splits"], plan["n_tiles"]
	assert S_ == _QT1_SPLITS and n_tiles == 1032 and n_tiles % S_ != 0 and n_tiles // S_ >= 3 and (n_tiles // S_) % 2 == 0, plan
	tiles = fx.sample_tiles(plan, I, leading, False)
	assert not set(_QT1_HOT) & set(tiles.tolist())
	X, E, S, (want_v, want_rows) = _qt1_case(Kp - 6)   # (K = 122 / 250: every k-step of the chain carries data)
	assert set((want_rows[0] // 32).tolist()) >= set(_QT1_HOT)   # every hot tile is in the answer
	Xp, Etp = fx.device_operands(ops, X, E.t(), Kp)
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws, **kw)
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(got_i, want_rows)
	# the threshold the sweep ran with (the k-th largest sampled group maximum, cut to its 16-bit key prefix) and who passes it
	gm = fx.reference_gmax(S, tiles, plan["group"])
	assert gm.shape[1] <= 4096
	tau = fx.coarse_floor(torch.topk(gm, k, dim=1).values[:, -1].numpy())
	hit = S.float() >= torch.from_numpy(tau)[:, None]
	# candidate segment of an item: (split = tile % splits, lane half = bit 2 of its row in the tile)
	item = torch.arange(I)
	seg = ((item // 32) % S_) * 2 + ((item % 32) >> 2 & 1)
	per_seg = torch.zeros(Q, 2 * S_, dtype=torch.int64).index_add_(1, seg, hit.long())
	assert int(per_seg.max()) <= plan["segment_capacity"] and int(per_seg.max()) >= 16, int(per_seg.max())
	assert int(nfb.item()) == 0, f"{int(nfb.item())} queries fell back although no segment overflows"
	surv = ops.fused_survivors(ws, Q, I, Kp, k, **kw) * Q
	assert round(surv) == int(hit.sum()) and abs(surv - round(surv)) < 1e-3, (surv, int(hit.sum()))


# ------------------------------------------------------------------ exact-integer fuzz
@settings(max_examples=_N or 40, deadline=None, derandomize=not _FUZZ, database=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(Q=st.integers(1, 300), I=st.integers(2500, 300000), K=st.integers(8, 256), kfrac=st.floats(0.0, 1.0), levels=st.integers(1, 3),
	   variant=st.sampled_from(["", "", "staged", "mfma16", "mfma32", "qt1"]), hints=st.booleans(),
	   kind=st.sampled_from(["ties", "const", "hot", "ascending"]), seed=st.integers(0, 10 ** 6))
def test_fused_exact_integer_fuzz(ops, Q, I, K, kfrac, levels, variant, hints, kind, seed):
	"""Small-integer operands over the shapes, k (up to 1024: ladder territory) and sweep variants of the Kp <= 256 path, with and without
	the index builder's hints (leading sample + item_ids, a random permutation: ties are then ordered by row, as the header says).
	Kinds: ties everywhere; one constant score (a flat ladder); whole tile ranges far above the sampled threshold; scores that grow with
	the row (every later tile beats the running threshold, and the leading sample holds the lowest).  THE top-k, bit for bit."""
	g = torch.Generator().manual_seed(seed)
	K = max(8, min(K, 40_000_000 // I))           # (bounded host work for the reference)
	Q = max(1, min(Q, 12_000_000 // I))
	Kp = ops.padded_k(K)
	k = 1 + int(kfrac * 1023)
	while k > 1 and not ops.fused_supported(Q, I, Kp, k):
		k //= 2
	if not ops.fused_supported(Q, I, Kp, k):
		return
	X = torch.randint(0, levels + 1, (Q, K), generator=g).float()
	if kind == "const":
		E = torch.ones(K, I)
	else:
		E = torch.randint(-levels, levels + 1, (K, I), generator=g).float()
	if kind == "hot":
		n_tiles = -(-I // 32)
		for _ in range(int(torch.randint(1, 4, (1,), generator=g))):
			w = int(torch.randint(1, max(2, n_tiles // 16), (1,), generator=g))
			t = int(torch.randint(0, max(1, n_tiles - w), (1,), generator=g))
			E[:, t * 32:(t + w) * 32] += levels + 1
	elif kind == "ascending":
		E += (torch.arange(I) * 8 // I).float()[None, :]
	S = (X @ E).long()                            # exact: integers below 2^24 at every partial sum
	kw = dict(mfma16=variant == "mfma16", qt1=variant == "qt1", mfma32=variant == "mfma32", staged=variant == "staged", leading_sample=hints)
	plan = ops.fused_plan(Q, I, Kp, k, **kw)
	if variant == "staged" or variant == "mfma32":
		assert not plan["ladder"]
	elif variant == "" and k <= 1024:
		assert plan["ladder"] and plan["lg"] == 1 and plan["n_stages"] == 1, plan
	perm = torch.randperm(I, generator=g).int() if hints else None
	Xp = ops.pack_bf16(X.cuda(), Kp)
	Etp = ops.pack_bf16(E.t().contiguous().cuda(), Kp, row_multiple=32)
	del E
	ws = ops.fused_workspace(Q, I, Kp, k, Xp.device)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, item_ids=perm.cuda() if hints else None, **kw)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, **kw) if plan["ladder"] else None
	want_v, want_rows = _reference(S, k)
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(got_i, perm.long()[want_rows] if hints else want_rows)
	if state is not None:
		_check_ladder(state, S, want_v[:, -1].numpy())
