"""The fused score + top-k when its sweep meets the prepass' sampled tiles LAST and starts the threshold ladder from the prepass
(csrc/score16.hpp 'SAMPLED TILES LAST'; the pre-credit: kth_value_wave_kernel in csrc/topk.hip; the chunk map: chunk_pos in csrc/sweep_common.hpp).

The route is taken by the ladder plans with the leading sample whose prepass runs on the sweep's own body (groups of 16: I >= 65 536 at
k <= 128); below that the plan keeps item order and counters from zero, and the same assertions hold for it.  All data is small-integer
(every bf16 operand and every fp32 sum exact), the reference is THE top-k from the host scores -- values descending, ties by ascending row --
and where a moved threshold could hide behind the select's rescan the ladder state itself is checked (test_gpu_fused_exact._check_ladder:
no level ever counts more items than exist at or above it; tau_final never above the true k-th score).
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_exact_cases as fx  # noqa: E402
import test_gpu_fused_exact as fe  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4          # CHUNK_TILES: tiles per ticket
I_RAGGED = 70001   # 2187 full tiles + 17 items: groups of 16 for k <= 129 (>= 8 x 258 full tiles), a partial last tile


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _sample_last(plan):
	"""The plan sweeps the sampled tiles last (plan_fused: P.sample_last > 0) -- given that the call passes leading_sample."""
	return plan["ladder"] and plan["group"] == 16


# ------------------------------------------------------------------ exactness across shapes
@functools.lru_cache(maxsize=2)
def _case(Q, I, K):
	X, E, S = fx.sparse_case(Q, I, K, seed=Q + I + K)
	return X, E, S


@functools.lru_cache(maxsize=4)
def _case_reference(Q, I, K, k):
	return fx.reference_topk(_case(Q, I, K)[2], k)


@pytest.mark.parametrize("ids", [False, True], ids=["rows", "item_ids"])
@pytest.mark.parametrize("Kp", [64, 256])
@pytest.mark.parametrize("I,k", [(60000, 1), (60000, 100), (60000, 128), (I_RAGGED, 1), (I_RAGGED, 100), (I_RAGGED, 128), (I_RAGGED, 129)])
@pytest.mark.parametrize("Q", [300, 17])
def test_sample_last_is_exact_across_shapes(ops, Q, I, k, Kp, ids):
	"""Two row blocks with a ragged second one / one short block; 1875 whole tiles (groups of 4: item order) / 2187 tiles and a partial one that
	now arrives mid-sequence (groups of 16: sampled tiles last); k = 129 samples 258 tiles, so the chunk that straddles the sample's end counts
	as sampled; with and without the index builder's id map."""
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=True)
	assert plan["ladder"] and plan["lg"] == 1 and plan["n_stages"] == 1, plan
	assert _sample_last(plan) == (I == I_RAGGED), plan
	if k == 129:
		assert plan["n_sample_tiles"] % CHUNK != 0, plan
	X, E, S = _case(Q, I, Kp - 6)
	want_v, want_rows = _case_reference(Q, I, Kp - 6, k)
	Xp, Etp = fx.device_operands(ops, X, E.t(), Kp)
	perm = torch.randperm(I, generator=torch.Generator().manual_seed(I + k)).int() if ids else None
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, leading_sample=True, item_ids=perm.cuda() if ids else None)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=True)
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(got_i, perm.long()[want_rows] if ids else want_rows)
	fe._check_ladder(state, S, want_v[:, -1].numpy())


# ------------------------------------------------------------------ pre-credit
def _highest_level_counts(gm, levels, k):
	"""[Q x 8]: group maxima gm [Q x G] per HIGHEST level reached (levels [Q x 8] ascending), each count capped at k; NaN reaches none."""
	with np.errstate(invalid="ignore"):
		h = (gm[:, :, None] >= levels[:, None, :]).sum(axis=2)
	return np.stack([np.minimum((h == j).sum(axis=1), k) for j in range(1, 9)], axis=1)


def test_precredit_matches_the_group_maxima():
	"""(host only) the reference of the next test counts each maximum once, at its highest level."""
	gm = np.array([[0., 1., 2., 8., 8., np.nan]])
	lv = np.arange(1, 9, dtype=np.float64)[None, :]
	assert _highest_level_counts(gm, lv, 100).tolist() == [[1, 1, 0, 0, 0, 0, 0, 2]]
	assert _highest_level_counts(gm, lv, 1).tolist() == [[1, 1, 0, 0, 0, 0, 0, 1]]


def test_precredit_counter_words(ops):
	"""Every item outside the 256 sampled tiles scores below zero and the sampled ones spread over [-48, 48], so the sweep keeps nothing it may count
	(sampled items are not counted) and the counter words it leaves are the threshold kernel's pre-credit: per query and level the group
	maxima whose highest reached level it is, capped at k.  Query 3 scores 0 everywhere (a flat ladder: all 512 maxima reach level 8, the
	field is capped at k, the sweep then counts the unsampled zeros on top), query 5 is NaN throughout (no maximum counts anywhere)."""
	Q, I, Kp, k, FLAT, NAN = 70, I_RAGGED, 64, 100, 3, 5
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=True)
	assert _sample_last(plan) and plan["n_sample_tiles"] == 256, plan
	n_samp = 256 * 32

	def plant(E, g):
		E[:, n_samp:] = -E[:, n_samp:].abs() - 1   # (coefficients are positive: every unsampled score is negative)

	X, E, S = fx.sparse_case(Q, I, Kp - 6, seed=11, plant=plant)
	X[FLAT] = 0
	S[FLAT] = 0
	Xn = X.clone()
	Xn[NAN] = float("nan")
	ok = np.array([q for q in range(Q) if q != NAN])
	assert int(S[:, n_samp:].max()) <= 0 and int(S[ok][:, n_samp:].min()) < 0
	Xp, Etp = fx.device_operands(ops, Xn, E.t(), Kp)
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, leading_sample=True)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=True)
	gm = fx.reference_gmax(S, fx.sample_tiles(plan, I, True, False), 16).double().numpy()
	# the ladder the threshold kernel built: tau0 = the k-th largest maximum (its 16-bit key prefix), levels above it
	kth_gm = np.sort(gm, axis=1)[:, ::-1][:, k - 1].astype(np.float32)
	assert (state["tau0"][ok] == fx.coarse_floor(kth_gm)[ok]).all()
	assert (state["tau0"][ok] > 0).sum() >= Q - 3 and state["tau0"][FLAT] == 0   # precondition: nothing unsampled passes (but the flat query's zeros)
	want = _highest_level_counts(gm, state["levels"].astype(np.float64), k)
	got = state["counts"].astype(np.int64)
	plain = np.array([q for q in ok if q != FLAT and state["tau0"][q] > 0])
	assert (got[plain] == want[plain]).all(), (got[plain][:2], want[plain][:2])
	assert len(plain) >= Q - 4 and (want[plain][:, :7] > 0).any() and (want[plain][:, 7] > 0).all()   # the case has something to count, below the top level too
	# flat ladder: every level equals tau0 = 0, all 512 maxima reach level 8 -> capped at k; the sweep adds unsampled zeros to the same field
	assert (state["levels"][FLAT] == 0).all() and want[FLAT].tolist() == [0] * 7 + [k]
	assert (got[FLAT][:7] == 0).all() and k <= got[FLAT][7] <= I
	# NaN row: no maximum counts
	assert (got[NAN] == 0).all(), got[NAN]
	want_v, want_rows = fx.reference_topk(S[ok], k)
	assert torch.equal(v.cpu()[ok].double(), want_v.double())
	assert torch.equal(i.cpu().long()[ok], want_rows)
	fe._check_ladder({key: a[ok] for key, a in state.items()}, S[ok], want_v[:, -1].numpy())


# ------------------------------------------------------------------ no double count
@pytest.mark.parametrize("where", ["sampled", "unsampled"])
@pytest.mark.parametrize("Kp", [256, 64])
@pytest.mark.parametrize("Q", [300, 1])
def test_sampled_items_are_not_counted_twice(ops, Q, Kp, where):
	"""k = 100.  'sampled': the only items at the ladder's top level (8) are 60 sampled ones, one per group; 39 more groups peak at 2..7 and the rest
	at 0 (99 groups above 0: tau0 = 0, the levels are 1..8); the unsampled tiles hold 30 000 items at 5 and zeros.  The pre-credit puts 60
	into the top field: counted once more by the sweep they would make 120 >= k, the threshold would move to 8 and the true k-th score -- 5 --
	would be cut (the select's rescan can hide that in the result, the ladder state cannot: level 8 would hold more counts than items exist).
	'unsampled': the mirror -- 50 items at 8 lie outside the sample, which peaks at 7 (30 groups) with 69 groups at 2..6.
	Kp = 256 is the case that bites: a build that goes on counting in the sampled chunks ends with 120 in the top field.  At Kp = 64 the queue's
	in-tile drain, which never counts, takes nearly every candidate (its limit is the empty queue there), so the ladder hardly counts at all."""
	I, k, n_st = I_RAGGED, 100, 256
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=True)
	assert _sample_last(plan) and plan["n_sample_tiles"] == n_st and plan["ladder_top_rank"] <= 30, plan
	s = np.zeros(I, dtype=np.int64)
	group_first = (np.arange(n_st)[:, None] * 32 + np.array([0, 4])[None, :]).ravel()   # rows 0 and 4 of a tile lie in its two groups
	top, n_top = (8, 60) if where == "sampled" else (7, 30)
	s[group_first[:n_top]] = top
	s[group_first[n_top:k - 1]] = 2 + np.arange(k - 1 - n_top) % (top - 2)   # 2 .. top - 1
	s[n_st * 32 + 2 * np.arange(30000)] = 5
	if where == "unsampled":
		s[n_st * 32 + 1 + 1000 * np.arange(50)] = 8
	Xp = torch.zeros((Q, Kp), dtype=torch.bfloat16, device="cuda")
	Xp[:, 0] = 1
	Etp = fe._etp_from_first_column(ops, s, Kp)
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws, leading_sample=True)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=True)
	assert (state["tau0"] == 0).all(), state["tau0"][:4]
	assert (state["levels"] == (top / 8) * np.arange(1, 9, dtype=np.float32)[None, :]).all(), state["levels"][:2]
	S = torch.from_numpy(s)[None, :]
	want_v, want_rows = fe._reference(S, k)
	assert int(want_v[0, -1]) == 5 and int((s >= 6).sum()) < k
	fe._check_ladder(state, S, 5.0)
	if where == "sampled":   # the pre-credit is there, and nothing was added to it
		assert (state["counts"][:, 7] == 60).all(), state["counts"][:2]
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double().expand(Q, k))
	assert torch.equal(got_i, want_rows.expand(Q, k))


# ------------------------------------------------------------------ repair path under the rotated chunk map
@pytest.mark.parametrize("pos", [5, 300, "last"])
def test_segment_overflow_is_repaired_under_the_rotated_chunk_map(ops, pos):
	"""One query scores its maximum on every item of ONE chunk of four tiles -- 128 (the last chunk: 113) candidates that no threshold can cut,
	in whichever workgroup draws that chunk, against a planned segment capacity of 64: that split's segment overflows and the select
	recomputes the tiles of the chunks the split owns, which it finds through the same chunk map as the sweep.  The chunk lies among the
	sampled tiles, in the middle of the matrix, or is the last one (its partial tile arrives mid-sequence)."""
	Q, I, Kp, k, Q0 = 17, I_RAGGED, 64, 10, 11
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=True)
	assert _sample_last(plan) and plan["lg"] == 1 and plan["segment_capacity"] == 64, plan
	n_chunks = -(-plan["n_tiles"] // CHUNK)
	p = n_chunks - 1 if pos == "last" else pos
	assert (p < plan["n_sample_tiles"] // CHUNK) == (pos == 5)
	K = Kp - 6
	g = torch.Generator().manual_seed(p)
	E = torch.randint(-8, 9, (K, I), generator=g).float()
	hot = slice(p * CHUNK * 32, min((p + 1) * CHUNK * 32, I))
	E[K - 1] = -1 - torch.randint(0, 250, (I,), generator=g).float()   # (spread out: about 1 item in 125 passes the query's first threshold, ~18 per segment)
	E[K - 1, hot] = 9
	Xs, _, _ = fx.sparse_x(Q, K - 1, g)
	X = torch.zeros(Q, K)
	X[:, :K - 1] = Xs
	X[Q0] = 0
	X[Q0, K - 1] = 1          # query Q0 reads row K - 1 of E alone, and nobody else reads it
	S = (X @ E).long()
	assert int(S[Q0].max()) == 9 and int((S[Q0] == 9).sum()) == hot.stop - hot.start > 64
	want_v, want_rows = fe._reference(S, k)
	Xp, Etp = fx.device_operands(ops, X, E.t(), Kp)
	ws = fx.poisoned_workspace(ops, Q, I, Kp, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws, leading_sample=True)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=True)
	assert int(nfb.item()) > 0
	got_i = i.cpu().long()
	assert ((got_i >= 0) & (got_i < I)).all()
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(got_i, want_rows)
	assert got_i[Q0].tolist() == list(range(hot.start, hot.start + k))
	fe._check_ladder(state, S, want_v[:, -1].numpy())
