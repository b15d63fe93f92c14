"""The prepass of the fused score + top-k on the sweep's 16x16x32 body (csrc/prepass16.hpp) and the workspace header the prepass kernels
clear themselves (zero_ws_header in csrc/sweep_common.hpp; there is no memset launch in front of the chain any more).

Every workspace here is filled with 0xff before its first call: the header words, the ticket counters and the ladder's counter words start
poisoned, so a chain that still relied on a memset returns garbage (tickets past the last chunk: nothing is swept; ladder fields at
65535: thresholds at the top level).  The group maxima are read back from the workspace (ops.fused_group_maxima) and compared BIT FOR BIT
with a host reference on exact integer data -- operands in [-8, 8], every inner product an integer below 2^15, exact in fp32 in any order --
in the layout the ladder tests pin: gmax[q, 2 j + g] = max over the 16 rows r of sample tile j with (r >> 2) & 1 == g.
Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _poisoned_workspace(ops, Q, I, Kp, k):
	ws = ops.fused_workspace(Q, I, Kp, k, torch.device("cuda"))
	ws.fill_(0xff)
	return ws


def _sample_tiles(plan, I, leading):
	n_full, n_st = I // 32, plan["n_sample_tiles"]
	j = np.arange(n_st, dtype=np.int64)
	return j if leading else (j * n_full) // n_st   # (the prepass' tile_of: the sample runs over the FULL tiles)


def _reference_gmax(X, E, tiles):
	"""X [Q x K], E [I x K] integer-valued float32 (CPU) -> [Q x 2 n_st] float32: the group maxima of the sampled tiles, group-16 layout."""
	rows = (torch.from_numpy(tiles)[:, None] * 32 + torch.arange(32)[None, :]).reshape(-1)
	S = X @ E[rows].t()                                   # exact: integers below 2^24
	S = S.view(X.shape[0], tiles.size, 32)
	g = (torch.arange(32) >> 2) & 1
	return torch.stack([S[:, :, g == 0].amax(dim=2), S[:, :, g == 1].amax(dim=2)], dim=2).reshape(X.shape[0], 2 * tiles.size)


def _reference_topk(S, k):
	"""THE top-k of integer scores S [Q x I] (int64): values descending, ties by ascending row."""
	I = S.shape[1]
	key = S * (1 << 27) - torch.arange(I, dtype=torch.int64)
	rows = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows), rows


def _integer_case(ops, Q, I, K, Kp, seed, padded_ldx):
	g = torch.Generator().manual_seed(seed)
	X = torch.randint(-8, 9, (Q, K), generator=g).float()
	E = torch.randint(-8, 9, (I, K), generator=g).float()
	Xp = ops.pack_bf16(X.cuda(), Kp)
	if padded_ldx:   # rows 16 elements apart from packed: ldx = Kp + 16 (a multiple of 8, 16-byte aligned), poison between the rows
		wide = torch.full((Q, Kp + 16), 7.0, dtype=torch.bfloat16, device="cuda")
		wide[:, :Kp] = Xp
		Xp = wide[:, :Kp]
		assert Xp.stride(0) == Kp + 16 or Q == 1
	Etp = ops.pack_bf16(E.cuda(), Kp, row_multiple=32)
	return X, E, Xp, Etp


def _bits(t):
	return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("leading", [True, False], ids=["leading", "strided"])
@pytest.mark.parametrize("tail", [1, 17, 31])
@pytest.mark.parametrize("Q", [1, 16, 255, 256, 257, 272])
@pytest.mark.parametrize("Kp", [64, 128, 256])
def test_prepass16_group_maxima_bit_exact_on_a_poisoned_workspace(ops, Kp, Q, tail, leading):
	"""Group maxima bit for bit, and THE top-k, from a workspace that starts as 0xff.  Q = 272: 16 valid rows in the last row block (as
	10 000 % 256 at the headline shape; that shape itself is the next test).  K is 8 short of Kp (zero-padded operands); every second
	tail runs with padded query rows."""
	K, I, k = Kp - 8, 2100 * 32 + tail, 100
	X, E, Xp, Etp = _integer_case(ops, Q, I, K, Kp, seed=Kp + 7 * Q + tail, padded_ldx=tail == 17)
	plan = ops.fused_plan(Q, I, Kp, k, leading_sample=leading)
	assert plan["group"] == 16 and plan["lg"] == 1 and plan["ladder"], plan
	ws = _poisoned_workspace(ops, Q, I, Kp, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws, leading_sample=leading)
	torch.cuda.synchronize()
	gmax, info = ops.fused_group_maxima(ws, Q, I, Kp, k, leading_sample=leading)
	assert info["prepass16"] and info["n_groups"] == 2 * plan["n_sample_tiles"], info
	want = _reference_gmax(X, E, _sample_tiles(plan, I, leading))
	got = gmax.cpu()
	assert got.shape == want.shape
	bad = (_bits(got) != _bits(want)).nonzero()
	assert bad.numel() == 0, f"{bad.shape[0]} group maxima differ; first (query, group) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
	# the chain behind it: THE top-k (stale tickets or ladder words would lose tiles or raise thresholds too far)
	want_v, want_rows = _reference_topk((X @ E.t()).long(), k)
	assert torch.equal(v.cpu().double(), want_v.double())
	assert torch.equal(i.cpu().long(), want_rows)
	# tau0 = the k-th largest group maximum, exactly (integers: the coarse threshold kernel has nothing to round)
	state = ops.fused_ladder_state(ws, Q, I, Kp, k, leading_sample=leading)
	assert (state["tau0"] <= want_v[:, -1].numpy()).all()
	assert (state["tau_final"] <= want_v[:, -1].numpy()).all()


def test_prepass16_group_maxima_at_the_headline_shape(ops):
	"""cfg2's shape (10 000 x 100 000, Kp = 256, k = 100: 40 row blocks, 16 valid rows in the last, 12 prepass splits): every group maximum
	bit for bit on a poisoned workspace, and no fallback."""
	Q, I, Kp, k = 10000, 100000, 256, 100
	X, E, Xp, Etp = _integer_case(ops, Q, I, Kp, Kp, seed=5, padded_ldx=False)
	plan = ops.fused_plan(Q, I, Kp, k)
	ws = _poisoned_workspace(ops, Q, I, Kp, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws)
	torch.cuda.synchronize()
	gmax, info = ops.fused_group_maxima(ws, Q, I, Kp, k)
	assert info["prepass16"] and info["prepass_splits"] > 1, info
	want = _reference_gmax(X, E, _sample_tiles(plan, I, False))
	assert torch.equal(_bits(gmax.cpu()), _bits(want))
	# the returned values are the items' true scores and none beats the k-th (spot check on a slice of the queries: the full matrix is 4 GB)
	sl = slice(9984, 10000)   # the last row block's 16 valid rows
	want_v, want_rows = _reference_topk((X[sl] @ E.t()).long(), k)
	assert torch.equal(v[sl].cpu().double(), want_v.double()) and torch.equal(i[sl].cpu().long(), want_rows)


def test_repeated_and_mixed_calls_on_one_workspace(ops):
	"""The same call twice on a poisoned-then-used workspace, then a small call after the large one on the same buffer: equal results and
	equal fallback counts (a stale ticket counter or ladder word would show as lost tiles or as thresholds that moved)."""
	Kp, k = 256, 100
	Ql, Il, Qs, Is = 700, 3000 * 32 + 17, 40, 2100 * 32 + 1
	Xl, El, Xpl, Etpl = _integer_case(ops, Ql, Il, Kp, Kp, seed=11, padded_ldx=False)
	Xs, Es, Xps, Etps = _integer_case(ops, Qs, Is, Kp, Kp, seed=12, padded_ldx=False)
	ws = _poisoned_workspace(ops, Ql, Il, Kp, k)
	assert ws.numel() >= ops.fused_workspace(Qs, Is, Kp, k, ws.device).numel()
	runs = []
	for _ in range(2):
		(v, i), nfb = ops.score_topk_fused(Xpl, Etpl, Il, k, return_fallbacks=True, workspace=ws)
		torch.cuda.synchronize()
		runs.append((v.cpu(), i.cpu(), int(nfb.item()), ops.fused_ladder_state(ws, Ql, Il, Kp, k)))
	assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] == 0
	assert np.array_equal(runs[0][3]["tau0"], runs[1][3]["tau0"]) and np.array_equal(runs[0][3]["levels"], runs[1][3]["levels"])
	want_v, want_rows = _reference_topk((Xl @ El.t()).long(), k)
	assert torch.equal(runs[1][0].double(), want_v.double()) and torch.equal(runs[1][1].long(), want_rows)
	# small after large, on the buffer the large call left behind -- against the same small call on a fresh poisoned workspace
	(v1, i1), nfb1 = ops.score_topk_fused(Xps, Etps, Is, k, return_fallbacks=True, workspace=ws)
	torch.cuda.synchronize()
	v1, i1, nfb1 = v1.cpu(), i1.cpu(), int(nfb1.item())
	(v2, i2), nfb2 = ops.score_topk_fused(Xps, Etps, Is, k, return_fallbacks=True, workspace=_poisoned_workspace(ops, Qs, Is, Kp, k))
	torch.cuda.synchronize()
	assert torch.equal(v1, v2.cpu()) and torch.equal(i1, i2.cpu()) and nfb1 == int(nfb2.item()) == 0
	want_v, want_rows = _reference_topk((Xs @ Es.t()).long(), k)
	assert torch.equal(v1.double(), want_v.double()) and torch.equal(i1.long(), want_rows)


@pytest.mark.parametrize("I", [60000, 100000])
def test_random_bf16_threshold_is_a_sweep_score_below_the_kth(ops, I):
	"""Random bf16 operands, cfg2-like (Q = 512, Kp = 256, k = 100).  I = 60 000 plans groups of 4 (the 32x32x16 prepass with the folded
	zeroing), I = 100 000 groups of 16 (the new kernel).  tau0 never exceeds the returned k-th value, nothing falls back, the top-k meets the
	fp64 reference within the tolerance of the parity tests (1e-4) -- and on the new kernel every group maximum above a query's k-th value
	appears BIT-EQUAL among the query's returned values: a group maximum is some sampled item's score, an item above the k-th is returned,
	and the returned values are the sweep's accumulators, so this holds exactly when both kernels accumulate alike."""
	Q, K, k, rank, noise = 512, 256, 100, 32, 0.05
	g = torch.Generator().manual_seed(I)
	Z = torch.randn(rank, I, generator=g)
	X = torch.randn(Q, K, generator=g).bfloat16()
	E = (torch.randn(K, rank, generator=g) @ Z / rank ** 0.5 + noise * torch.randn(K, I, generator=g)).bfloat16()
	Xp = ops.pack_bf16(X.cuda(), K)
	Etp = ops.pack_bf16(E.t().contiguous().cuda(), K, row_multiple=32)
	plan = ops.fused_plan(Q, I, K, k)
	assert plan["ladder"], plan
	ws = _poisoned_workspace(ops, Q, I, K, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws)
	torch.cuda.synchronize()
	assert nfb.item() == 0
	state = ops.fused_ladder_state(ws, Q, I, K, k)
	vc = v.cpu()
	assert (torch.from_numpy(state["tau0"]) <= vc[:, k - 1]).all()
	S = X.double() @ E.double()
	rv, ri = torch.topk(S, k, dim=1)
	torch.testing.assert_close(vc.double(), rv, rtol=1e-4, atol=1e-4)
	got = i.cpu().long()
	assert (got >= 0).all() and (got < I).all()
	torch.testing.assert_close(torch.gather(S, 1, got), vc.double(), rtol=1e-4, atol=1e-4)
	gmax, info = ops.fused_group_maxima(ws, Q, I, K, k)
	assert info["prepass16"] == (plan["group"] == 16) == (I == 100000), (info, plan)
	if info["prepass16"]:
		gm = gmax.cpu()
		n_above = 0
		for q in range(Q):
			above = gm[q][gm[q] > vc[q, k - 1]]
			n_above += above.numel()
			missing = above[~torch.isin(_bits(above), _bits(vc[q]))]
			assert missing.numel() == 0, f"query {q}: group maxima {missing[:4].tolist()} beat the k-th value but are not among the returned values bit for bit"
		assert n_above >= Q   # the check saw something: the sample holds about 8 % of each query's top 100


def test_eval_fused_and_kp512_on_a_poisoned_workspace(ops):
	"""The 32x32x16 prepass with the folded zeroing: the one-pass evaluation route (evalf plan, static shares) and a Kp = 512 call (wave-queue
	body with sliced tickets), both on workspaces that start as 0xff, against the routes that do not depend on the header."""
	# eval_fused takes the shared grow-only workspace: size it, poison it
	Q, I, K, k = 300, 70001, 200, 100
	g = torch.Generator().manual_seed(3)
	X = torch.randint(-8, 9, (Q, K), generator=g).float()
	E = torch.randint(-8, 9, (I, K), generator=g).float()
	Kp = ops.padded_k(K)
	Xp = ops.pack_bf16(X.cuda(), Kp)
	Etp = ops.pack_bf16(E.cuda(), Kp, row_multiple=32)
	S = X @ E.t()
	A = (S + torch.randint(-3, 4, S.shape, generator=g).float()).bfloat16()   # (rounded to bf16: the reference sums below use the rounded values)
	Ad = torch.zeros((Q, -(-I // 8) * 8), dtype=torch.bfloat16, device="cuda")[:, :I]
	Ad.copy_(A)
	assert ops.eval_fused_ok(Kp, Ad, Q, I, k)
	from anncur_amd import _lib
	nbytes = _lib.load().anncur_eval_fused_workspace_bytes(Q, I, Kp, k)
	ops._Workspace.get(nbytes, Xp.device).fill_(0xff)
	(v, i), err, nrm, nfb = ops.eval_fused(Xp, Etp, Ad, I, k, return_fallbacks=True)
	torch.cuda.synchronize()
	assert nfb.item() == 0
	want_v, want_rows = _reference_topk(S.long(), k)
	assert torch.equal(v.cpu().double(), want_v.double()) and torch.equal(i.cpu().long(), want_rows)
	# the two sums are fp32 accumulations of I = 70 001 non-negative terms (exact terms: S and A are integers): relative error at most
	# I x 2^-24 = 4e-3 in the worst order, about sqrt(I) x 2^-24 = 2e-5 for partial sums per lane; 1e-4 sits between the two
	Af = A.double()
	torch.testing.assert_close(err.cpu().double(), ((S.double() - Af) ** 2).sum(1), rtol=1e-4, atol=0)
	torch.testing.assert_close(nrm.cpu().double(), (Af ** 2).sum(1), rtol=1e-4, atol=0)
	# Kp = 512
	Q, I, K, k = 130, 2100 * 32 + 17, 500, 64
	X = torch.randint(-8, 9, (Q, K), generator=g).float()
	E = torch.randint(-8, 9, (I, K), generator=g).float()
	Xp = ops.pack_bf16(X.cuda(), 512)
	Etp = ops.pack_bf16(E.cuda(), 512, row_multiple=32)
	ws = _poisoned_workspace(ops, Q, I, 512, k)
	(v, i), nfb = ops.score_topk_fused(Xp, Etp, I, k, return_fallbacks=True, workspace=ws)
	torch.cuda.synchronize()
	assert nfb.item() == 0
	_, info = ops.fused_group_maxima(ws, Q, I, 512, k)
	assert not info["prepass16"]
	want_v, want_rows = _reference_topk((X @ E.t()).long(), k)
	assert torch.equal(v.cpu().double(), want_v.double()) and torch.equal(i.cpu().long(), want_rows)
