"""Exact-data tests of the small-batch route (csrc/few.hip): ops.score_rows_few (launch 1: every score and every group maximum)
and ops.score_topk_few (both launches: values, ids and the select's counters).

The data are small integers (tests/fused_exact_cases.py), so every bf16 operand and every fp32 partial sum is exact in any order, and the host
references -- integer matrix products, tests/topk_numpy.py, the numpy model of the select in tests/few_numpy.py -- never read the device.  All
comparisons are bit for bit.  Two constructions beside dense_case:
  * identity queries: X[q] = e_q makes S[q, i] = E[i, q], so a test writes the score row it wants (planted winners, a group whose maximum
    is exactly the threshold) straight into E;
  * one-hot items: item i = e_(i mod K) makes S[q, i] = X[q, i mod K], so every (item row, k position, query column) of the MFMA fragment
    mapping shows in S."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import few_numpy as fn  # noqa: E402
import fused_exact_cases as fx  # noqa: E402
from fused_exact_cases import dense_case, device_operands, reference_topk, sparse_case  # noqa: E402
from topk_numpy import topk_ref  # noqa: E402

pytestmark = pytest.mark.gpu
QS = (1, 15, 16, 17, 33, 64)
IS = (1, 15, 16, 17, 63, 64, 65, 4101)


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _bits_equal(got, want, what):
	g, w = got.detach().cpu().contiguous(), torch.as_tensor(want).contiguous()
	assert g.shape == w.shape, (what, g.shape, w.shape)
	if g.dtype == torch.float32:
		w = w.to(torch.float32)
		ok = (g.view(torch.int32) == w.view(torch.int32)) | (g.isnan() & w.isnan())
	else:
		ok = g.to(torch.int64) == w.to(torch.int64)
	bad = (~ok).nonzero()
	assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def _check_rows(ops, Xp, Etp, S, what):
	"""score_rows_few against host scores S [Q x I] (float32 tensor): every score, every group maximum."""
	I = S.shape[1]
	got_S, got_GM = ops.score_rows_few(Xp, Etp, I)
	torch.cuda.synchronize()
	_bits_equal(got_S, S, f"{what}: S")
	with np.errstate(invalid="ignore"):
		_bits_equal(got_GM, torch.from_numpy(fn.group_maxima(S.numpy())), f"{what}: GM")


def _check_topk(ops, Xp, Etp, S, k, what, want=None, expect_fallback=0):
	"""score_topk_few on a 0xff-filled workspace against the reference top-k and the model's counters.  S: host scores [Q x I], integer
	tensor (reference_topk) or float32 with non-finite entries (topk_ref per row)."""
	Q, I = S.shape
	Kp = Xp.shape[1]
	ws = ops.few_workspace(Q, I, Kp, k, torch.device("cuda"))
	ws.fill_(0xff)
	got, st = ops.score_topk_few(Xp, Etp, I, k, workspace=ws, return_stats=True)
	torch.cuda.synchronize()
	Sf = S.float().numpy()
	if want is None:
		if S.dtype.is_floating_point:
			ref = [topk_ref(Sf[q], k) for q in range(Q)]
			want = (torch.from_numpy(np.stack([r[0] for r in ref])), torch.from_numpy(np.stack([r[1] for r in ref])))
		else:
			want = reference_topk(S, k)
	_bits_equal(got.values, want[0].float(), f"{what}: values")
	_bits_equal(got.indices, want[1], f"{what}: ids")
	model = [fn.select_model(Sf[q], k)[2] for q in range(Q)]
	cap = ops.few_plan(Q, I, Kp, k)["cand_cap"]
	assert cap == fn.cand_cap(k)
	for name, dev in zip(("groups_read", "n_cand", "fallback"), st):
		_bits_equal(dev, torch.tensor([m[name] for m in model]), f"{what}: {name}")
	if expect_fallback is not None:
		assert all(m["fallback"] == expect_fallback for m in model), (what, model)
		if not expect_fallback:
			assert all(m["n_cand"] <= cap for m in model)
	return model


def _identity_case(ops, S, Kp):
	"""Operands whose scores are the given integers S [Q x I] (|S| <= 256, Q <= Kp): X[q] = e_q, E[i, q] = S[q, i]."""
	Q, I = S.shape
	assert Q <= Kp and int(S.abs().max()) <= 256
	E = torch.zeros(I, Kp)
	E[:, :Q] = S.t().float()
	return device_operands(ops, torch.eye(Q, Kp), E, Kp)


# ================================================================== launch 1: all scores
def _widest_kp(ops, Q):
	return max(kp for kp in [64, 128, 256, 512] + list(range(640, 4097, 128)) if ops.score_topk_few_ok(Q, 1000, kp, 1))


@pytest.mark.parametrize("Kp,dk", [(kp, dk) for kp in (64, 128, 256, 512) for dk in (0, 3)])
def test_all_scores(ops, Kp, dk):
	K = Kp - dk
	plan_I = 64 * 9 + 16 + 5      # ten groups: one wave each, the last wave two tiles, the second of them ragged
	p = ops.few_plan(64, plan_I, Kp, 1)
	assert p["tiles_per_wave_min"] >= 2 and p["tiles"] * 16 > plan_I and p["workgroups"] > 1
	X, E, S = dense_case(64, 4101, K, seed=Kp + dk)
	for Q in QS:
		for I in IS + (plan_I,):
			Xp, Etp = device_operands(ops, X[:Q], E[:I], Kp)
			_check_rows(ops, Xp, Etp, S[:Q, :I].float(), f"Q={Q} I={I} Kp={Kp} K={K}")


@pytest.mark.parametrize("dk", [0, 3])
def test_all_scores_at_the_widest_kp_of_16_queries(ops, dk):
	Kp = _widest_kp(ops, 16)
	assert Kp == 2048 and not ops.score_topk_few_ok(17, 1000, Kp, 1)
	X, E, S = dense_case(16, 4101, Kp - dk, seed=dk)
	for Q, I in ((16, 4101), (1, 65), (15, 597)):
		Xp, Etp = device_operands(ops, X[:Q], E[:I], Kp)
		_check_rows(ops, Xp, Etp, S[:Q, :I].float(), f"Q={Q} I={I} Kp={Kp}")
	for Kw, Q in ((640, 48), (1024, 32)):      # the other wide widths, at the most queries each admits
		assert ops.score_topk_few_ok(Q, 1000, Kw, 1) and not ops.score_topk_few_ok(Q + 1, 1000, Kw, 1)
		X, E, S = dense_case(Q, 1029, Kw - 5, seed=Kw)
		Xp, Etp = device_operands(ops, X, E, Kw)
		_check_rows(ops, Xp, Etp, S.float(), f"Q={Q} Kp={Kw}")


def test_all_scores_with_several_groups_per_wave(ops):
	I = 64 * 2048 * 2 + 64 * 3 + 16 + 5
	p = ops.few_plan(3, I, 64, 1)
	assert p["groups_per_wave"] == 3 and p["tiles_per_wave_max"] == 12 and 2 <= p["tiles_per_wave_min"] < 12 and I % 16
	X, E, S = dense_case(3, I, 61, seed=5)
	Xp, Etp = device_operands(ops, X, E, 64)
	_check_rows(ops, Xp, Etp, S.float(), "three groups per wave")


@pytest.mark.parametrize("Kp", [64, 128, 256, 512, 640])
def test_one_hot_items_show_the_fragment_mapping(ops, Kp):
	K, Q = Kp - 3, 64 if Kp <= 512 else 48
	I = 4 * K + 5
	d = torch.arange(K)
	X = ((d[None, :] * 7 + torch.arange(Q)[:, None] * 3) % 256 - 128).float()      # a different integer for every (query, dimension) residue
	E = torch.zeros(I, K)
	E[torch.arange(I), torch.arange(I) % K] = 1.0
	Xp, Etp = device_operands(ops, X, E, Kp)
	_check_rows(ops, Xp, Etp, X[:, torch.arange(I) % K], f"one-hot Kp={Kp}")


# ================================================================== both launches: top-k
@pytest.mark.parametrize("I,k", [(4101, 100), (16421, 100), (16421, 1), (16421, 128), (16421, 129), (200005, 1024), (4101, 1024), (100, 100), (17, 17), (1, 1)])
def test_topk_dense(ops, I, k):
	"""4101 items are 65 groups < k = 100: no threshold, every item a candidate, still under the cap; 16421 are 257 groups."""
	for Q, Kp in ((5, 64), (17, 256)):
		X, E, S = dense_case(Q, I, Kp - 3, seed=I + k)
		Xp, Etp = device_operands(ops, X, E, Kp)
		model = _check_topk(ops, Xp, Etp, S, k, f"I={I} k={k} Q={Q} Kp={Kp}")
		if -(-I // 64) < k:
			assert all(m["tau"] == -np.inf and m["n_cand"] == I for m in model)


@pytest.mark.parametrize("k", [1, 100, 129])
def test_topk_tie_heavy_rows_take_the_smaller_id(ops, k):
	X, E, S = dense_case(33, 16421, 61, seed=k, xmax=1, emax=1)
	Xp, Etp = device_operands(ops, X, E, 64)
	_check_topk(ops, Xp, Etp, S, k, f"ties k={k}")
	Xs, Es, Ss = sparse_case(9, 16421, 128, seed=k)
	Xp, Etp = device_operands(ops, Xs, Es.t(), 128)
	_check_topk(ops, Xp, Etp, Ss, k, f"sparse k={k}")


def test_topk_planted_winners(ops):
	I, k, Q = 16421, 100, 6
	g = torch.Generator().manual_seed(1)
	S = torch.randint(-5, 6, (Q, I), generator=g)
	plant = [0, 15, 16, 31, 63, 64, 16 * 500, 16 * 500 + 15, 64 * 200, 64 * 200 + 63, I - 2, I - 1]      # first / last of a tile, of a group, of the row
	for q in range(Q):
		for j, i in enumerate(plant):
			S[q, i] = 250 - 2 * ((j + q) % len(plant))
	# one item in 20..199 in each of 95 more groups: 100 groups reach the threshold, 107 items do, the twelve planted ones lead
	free = [gr for gr in range(257) if all(i // 64 != gr for i in plant)]
	assert len({i // 64 for i in plant}) == 5
	for q in range(Q):
		pick = torch.randperm(len(free), generator=g)[:95]
		for j, f in enumerate(pick.tolist()):
			S[q, free[f] * 64 + (j * 13 + q) % 64] = 20 + (j * 2) % 180
	Xp, Etp = _identity_case(ops, S, 64)
	model = _check_topk(ops, Xp, Etp, S, k, "planted")
	want_i = reference_topk(S, k)[1]
	assert all(m["tau"] >= 20 and m["groups_read"] == 100 and m["n_cand"] == 107 for m in model)
	for q in range(Q):
		assert set(plant) <= set(want_i[q].tolist())


def test_topk_winner_in_the_group_whose_maximum_is_the_threshold(ops):
	"""100 groups hold one item above the bulk each, and the weakest of them, item 77 * 64 + 40, scores exactly 10: with k = 100 the threshold
	is that group's maximum and the item is the k-th result."""
	I, k, Q = 16421, 100, 4
	g = torch.Generator().manual_seed(2)
	S = torch.randint(-5, 6, (Q, I), generator=g)
	free = [gr for gr in range(257) if gr != 77]
	for q in range(Q):
		pick = torch.randperm(len(free), generator=g)[:99]
		for j, f in enumerate(pick.tolist()):
			S[q, min(free[f] * 64 + (j * 13 + q) % 64, I - 1)] = 20 + (j * 2) % 180
		S[q, 77 * 64 + 40] = 10
	Xp, Etp = _identity_case(ops, S, 64)
	model = _check_topk(ops, Xp, Etp, S, k, "threshold group")
	want_v, want_i = reference_topk(S, k)
	assert all(m["tau"] == 10 and m["groups_read"] == 100 and m["n_cand"] == 100 for m in model)
	assert (want_i[:, -1] == 77 * 64 + 40).all() and (want_v[:, -1] == 10).all()


def test_every_score_ties_falls_back_and_stays_exact(ops):
	Q, I = 7, 20000
	X, E, S = dense_case(Q, I, 61, seed=2, const=True)
	Xp, Etp = device_operands(ops, X, E, 64)
	for k in (1, 100, 1024):
		ws = ops.few_workspace(Q, I, 64, k, torch.device("cuda"))
		ws.fill_(0xff)
		got, st = ops.score_topk_few(Xp, Etp, I, k, workspace=ws, return_stats=True)
		torch.cuda.synchronize()
		assert st.fallback.cpu().tolist() == [1] * Q and st.n_cand.cpu().tolist() == [I] * Q
		_bits_equal(got.indices, torch.arange(k).expand(Q, k), "ids 0..k-1")
		_bits_equal(got.values, S[:, :1].float().expand(Q, k), "the one value")
		_check_topk(ops, Xp, Etp, S, k, f"const k={k}", expect_fallback=1)


# ================================================================== layout hygiene, refusals
def test_pitched_queries_poisoned_workspace_and_guards(ops):
	from anncur_amd import _lib
	Q, I, Kp, k = 17, 4101, 128, 100
	X, E, S = dense_case(Q, I, Kp - 3, seed=9)
	Xp, Etp = device_operands(ops, X, E, Kp, ldx_pad=8)
	assert Xp.stride(0) == Kp + 8
	_check_rows(ops, Xp, Etp, S.float(), "pitched X")
	_check_topk(ops, Xp, Etp, S, k, "pitched X")
	lib = _lib.load()
	nbytes = lib.anncur_score_topk_few_workspace_bytes(Q, I, Kp, k)
	G = 4096
	buf = torch.full((nbytes + 256 + G,), 0xff, dtype=torch.uint8, device="cuda")
	off = (-buf.data_ptr()) % 256
	val = torch.full((Q * k + G,), -1, dtype=torch.int32, device="cuda")
	idx = torch.full((Q * k + G,), -1, dtype=torch.int32, device="cuda")
	_lib.check(lib.anncur_score_topk_few(ops._p(Xp), Xp.stride(0), ops._p(Etp), Kp, Q, I, Kp, k, ops._p(val), ops._p(idx), ops._p(buf[off:]), nbytes, ops._stream()),
			   "score_topk_few")
	torch.cuda.synchronize()
	want_v, want_i = reference_topk(S, k)
	_bits_equal(val[:Q * k].view(torch.float32).view(Q, k), want_v.float(), "values")
	_bits_equal(idx[:Q * k].view(Q, k), want_i, "ids")
	assert (val[Q * k:] == -1).all() and (idx[Q * k:] == -1).all(), "guard behind an output"
	assert (buf[:off] == 0xff).all() and (buf[off + nbytes:] == 0xff).all(), "guard around the workspace"
	hdr = buf[off:off + 1024].view(torch.int32).view(64, 4)
	assert not hdr[Q:].any() and not hdr[:, 3].any() and not hdr[:Q, 2].any(), "header rows past Q are zero"
	# score_rows_few writes nothing outside [Q x I] and [Q x ceil(I / 64)]
	pitch, ng = -(-I // 32) * 32, -(-I // 64)
	Sb = torch.full((Q * pitch + G,), -1, dtype=torch.int32, device="cuda")
	Gb = torch.full((Q * (ng + 3) + G,), -1, dtype=torch.int32, device="cuda")
	_lib.check(lib.anncur_score_rows_few(ops._p(Xp), Xp.stride(0), ops._p(Etp), Kp, Q, I, Kp, ops._p(Sb), pitch, ops._p(Gb), ng + 3, ops._stream()), "score_rows_few")
	torch.cuda.synchronize()
	Sv, Gv = Sb[:Q * pitch].view(Q, pitch), Gb[:Q * (ng + 3)].view(Q, ng + 3)
	_bits_equal(Sv[:, :I].view(torch.float32), S.float(), "S")
	assert (Sv[:, I:] == -1).all() and (Sb[Q * pitch:] == -1).all() and (Gv[:, ng:] == -1).all() and (Gb[Q * (ng + 3):] == -1).all()


def test_refusals_name_the_limit(ops):
	from anncur_amd import _lib
	X, E, S = dense_case(65, 1000, 61, seed=3)
	Xp, Etp = device_operands(ops, X, E, 64)
	with pytest.raises(ValueError, match=r"Q = 65 .*1\.\.64"):
		ops.score_topk_few(Xp, Etp, 1000, 10)
	with pytest.raises(ValueError, match=r"k = 1001 .*= 1000"):
		ops.score_topk_few(Xp[:4], Etp, 1000, 1001)
	with pytest.raises(ValueError, match=r"k = 2049 .*= 2048"):
		ops.score_topk_few(Xp[:4], torch.zeros((4128, 64), dtype=torch.bfloat16, device="cuda"), 4101, 2049)
	odd = torch.zeros((4, 68), dtype=torch.bfloat16, device="cuda")[:, :64]
	with pytest.raises(ValueError, match=r"ldx = 68.*multiple of 8"):
		ops.score_topk_few(odd, Etp, 1000, 10)
	# the library refuses the same on its own
	lib = _lib.load()
	out_v, out_i = torch.empty(65 * 10, device="cuda"), torch.empty(65 * 10, dtype=torch.int32, device="cuda")
	ws = ops.few_workspace(64, 1000, 64, 10, torch.device("cuda"))
	for args, word in (((65, 1000, 64, 10), "1..64"), ((4, 1000, 64, 1001), "min(I = 1000, 2048)")):
		rc = lib.anncur_score_topk_few(ops._p(Xp), 64, ops._p(Etp), 64, *args, ops._p(out_v), ops._p(out_i), ops._p(ws), ws.numel(), ops._stream())
		assert rc < 0 and word in lib.anncur_last_error().decode()
	rc = lib.anncur_score_topk_few(ops._p(Xp), 68, ops._p(Etp), 64, 4, 1000, 64, 10, ops._p(out_v), ops._p(out_i), ops._p(ws), ws.numel(), ops._stream())
	assert rc < 0 and "multiple of 8" in lib.anncur_last_error().decode()
	rc = lib.anncur_score_topk_few(ops._p(Xp), 64, ops._p(Etp), 64, 4, 1000, 64, 10, ops._p(out_v), ops._p(out_i), ops._p(ws), 1024, ops._stream())
	assert rc == -2 and "workspace" in lib.anncur_last_error().decode()


# ================================================================== non-finite scores
def _f64_scores(X, E):
	"""float64 products, summed; NaN / inf follow IEEE in any order (a sum that meets +inf and -inf, inf . 0, a NaN factor: NaN)."""
	with np.errstate(invalid="ignore", over="ignore"):
		P = X.double().numpy()[:, None, :] * E.double().numpy()[None, :, :]
		return torch.from_numpy(P.sum(axis=2).astype(np.float32))


def test_non_finite_scores(ops):
	Q, I, K, Kp, k = 17, 4101, 29, 64, 100
	X, E, _ = dense_case(Q, I, K, seed=11)
	X[:, 0] = torch.tensor([0.0, 1.0, 2.0] * 6)[:Q]          # column 0 decides what an infinite item entry gives: inf . 0 = NaN, else inf
	nan, inf = float("nan"), float("inf")
	E[0], E[I - 1], E[700], E[64 * 20:64 * 21] = nan, nan, nan, nan      # item 0, item I - 1, inside a group, a whole group
	E[5] = 0
	E[5, 0] = inf                                              # +inf for the queries with X[q, 0] > 0, NaN for the others
	E[4000] = 0
	E[4000, 0] = -inf
	E[1234, 0], E[1234, 1] = inf, -inf                         # +inf - inf (or NaN factors): NaN wherever both columns are non-zero
	X[3] = nan                                                 # a NaN query row inside sub-tile 0: k pads, its neighbours stay exact
	S = _f64_scores(X, E)
	assert S[3].isnan().all() and S[1, 5] == inf and S[0, 5].isnan() and S[1, 4000] == -inf and S[:, 0].isnan().all()
	Xp, Etp = device_operands(ops, X, E, Kp)
	_check_rows(ops, Xp, Etp, S, "non-finite")
	model = _check_topk(ops, Xp, Etp, S, k, "non-finite")
	got = ops.score_topk_few(Xp, Etp, I, k)
	assert (got.indices[3] == -1).all() and got.values[3].isneginf().all() and model[3]["groups_read"] == 0
	assert not torch.isin(got.indices.cpu(), torch.tensor([0, I - 1, 700])).any()
	assert (got.indices[[1, 2, 4], 0] == 5).all()
	# fewer than k non-NaN scores: them, then pads (Q = 2: one such query beside an ordinary one)
	X2, E2, _ = dense_case(2, 300, K, seed=12)
	E2[:] = nan
	E2[[3, 100, 299]] = torch.tensor([[1.0], [-2.0], [2.0]]).expand(3, K)
	S2 = _f64_scores(X2, E2)
	Xp, Etp = device_operands(ops, X2, E2, Kp)
	_check_topk(ops, Xp, Etp, S2, 10, "three real scores")
	got = ops.score_topk_few(Xp, Etp, 300, 10)
	assert (got.indices[:, 3:] == -1).all() and got.values[:, 3:].isneginf().all() and sorted(got.indices[0, :3].tolist()) == [3, 100, 299]


# ================================================================== an item matrix beyond 2^31 elements
def test_item_rows_beyond_32_bit_offsets(ops):
	"""Q = 1, Kp = 512, 2^31 + 101 * 512 elements of Et inside a 0xff-filled allocation (NaN as bf16); the bulk and the query as _big_case of
	tests/test_gpu_far_rows_exact.py.  Winners planted on both sides of byte 2^31 (row 2^21) and byte 2^32 (row 2^22 = element 2^31)."""
	torch.cuda.empty_cache()
	Kp, k = 512, 10
	I = (1 << 31) // Kp + 101
	Ip = -(-I // 32) * 32
	r31, r32 = (1 << 31) // (2 * Kp), (1 << 32) // (2 * Kp)
	assert ops.score_topk_few_ok(1, I, Kp, k) and I % 16 and r32 * Kp == 1 << 31 < I * Kp
	guard = 1 << 20
	buf = torch.empty(Ip * Kp + 2 * guard, dtype=torch.int16, device="cuda")
	buf.fill_(-1)
	E = buf[guard:guard + Ip * Kp].view(torch.bfloat16).view(Ip, Kp)
	torch.manual_seed(1)
	for r0 in range(0, Ip, 1 << 20):
		r1 = min(Ip, r0 + (1 << 20))
		E[r0:r1] = torch.randint(-100, 101, (r1 - r0, Kp), device="cuda", dtype=torch.int8).to(torch.bfloat16)
	E[I:] = 0
	plant = torch.tensor([0, 15, r31 - 1, r31, r32 - 1, r32, r32 + 40, I - 2, I - 1, 1000])
	assert plant.unique().numel() == k and r32 + 40 < I - 2
	order = (torch.arange(k) * 7) % k                                                    # planted item j is the order[j]-th best
	E[plant.cuda(), 0] = (200 - 2 * order).to(torch.bfloat16).cuda()
	E[plant.cuda(), 32] = 0
	X = torch.zeros((1, Kp), dtype=torch.bfloat16, device="cuda")
	X[0, 0], X[0, 32] = 1, 2.0 ** -8                                                     # bulk scores E[i, 0] + E[i, 32] / 256: exact, below 101
	ws = ops.few_workspace(1, I, Kp, k, torch.device("cuda"))
	ws.fill_(0xff)
	got, st = ops.score_topk_few(X, E, I, k, workspace=ws, return_stats=True)
	torch.cuda.synchronize()
	_bits_equal(got.values, (200 - 2 * torch.arange(k)).float()[None, :], "values")
	_bits_equal(got.indices, plant[torch.argsort(order)][None, :], "items")
	assert st.fallback.item() == 0 and st.groups_read.item() >= k
	S, GM = ops.score_rows_few(X, E, I)
	torch.cuda.synchronize()
	_bits_equal(S[0, plant.cuda()], (200 - 2 * order).float(), "scores of the planted items")
	assert S.shape == (1, I) and not S.isnan().any() and S.abs().max().item() == 200.0 and GM.shape == (1, -(-I // 64))
	assert order[0] == 0 and GM[0, 0].item() == 200.0      # the best item's group maximum
	assert (buf[:guard] == -1).all() and (buf[guard + Ip * Kp:] == -1).all()
	del S, GM, E, buf, ws
	torch.cuda.empty_cache()
