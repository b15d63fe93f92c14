"""The split-bf16 ("bf16x3") route: anncur_pack_split_bf16, anncur_rescore_topk, the fused sweep on the split operands, and the
route end to end through CURRowIndex / FlatIPIndex / both CLIs.

References are int64 / fp64 CPU arithmetic, a numpy restatement of the split written here, or the existing dense fp32 route
(ops.gemm + the exact scan) -- never the code under test.

Error bound of the split scores: |x - hi| <= 2^-9 |x|, |x - hi - lo| <= 2^-18 |x|, the dropped product
|lo_x lo_e| <= 2^-18 |x||e|: each term is off by at most 3 2^-18 |x_k||e_k| before accumulation, the fp32 sum of 3K terms adds about
3K 2^-24 sum |x_k||e_k|.  The tests hold  |S_split - S_fp64| <= (2^-16 + 3K 2^-23) (|X|.|E|^T)[q, i]  (2.6x / 2x the two terms).

Smallest item counts the fused path takes (anncur_score_topk_supported, found on the host): 8192 up to k = 116, 8320 at k = 130,
9344 at k = 146 for Kp = 256 / 512; 4096 / 4608 / 5120 for Kp = 768.  One ragged count above all of them serves every case.
Needs an MI355X."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ITEMS = 9371   # >= 9344, not a multiple of 32


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


# ------------------------------------------------------------------ numpy restatement of the split
def _rne_bf16_bits(x):
	"""float32 array -> bf16 bit patterns (uint16), round-to-nearest-even, NaN stays (quiet) NaN."""
	u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
	nan = (u & 0x7fffffff) > 0x7f800000
	r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
	return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def _bf16_bits_to_f32(b):
	return (b.astype(np.uint32) << 16).view(np.float32)


def _split_bits(x):
	"""(hi, lo) bf16 bit patterns of a float32 array: hi = RNE(x), lo = RNE(x - hi), lo = 0 where hi is not finite."""
	hi = _rne_bf16_bits(x)
	finite = (hi & 0x7f80) != 0x7f80
	with np.errstate(invalid="ignore", over="ignore"):
		d = np.where(finite, x.astype(np.float32) - _bf16_bits_to_f32(hi), np.float32(0))   # exact in fp32
	lo = np.where(finite, _rne_bf16_bits(d.astype(np.float32)), 0).astype(np.uint16)
	return hi, lo


def _pack_split_np(hi, lo, role, Kp, n_pad):
	n, K = hi.shape
	out = np.zeros((n_pad, Kp), dtype=np.uint16)
	segs = (lo, hi, hi) if role == 0 else (hi, lo, hi)
	for s, seg in enumerate(segs):
		out[:n, s * K:(s + 1) * K] = seg
	return out


def _bits(t):
	return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _special_values(n, K, seed):
	"""fp32 [n x K]: normals across many exponents, subnormals, +-0, +-inf, NaN, a finite value that rounds to bf16 inf, and RNE ties
	(x - hi exactly half an ulp of hi, hi's last bit even and odd)."""
	rng = np.random.default_rng(seed)
	x = (rng.standard_normal(n * K) * np.exp2(rng.integers(-120, 120, n * K))).astype(np.float32)
	sub = (rng.integers(1, 1 << 23, n * K).astype(np.uint32) | (rng.integers(0, 2, n * K).astype(np.uint32) << 31)).view(np.float32)
	tie = ((rng.integers(0x0080, 0x7f7f, n * K).astype(np.uint32) << 16) | 0x8000 | (rng.integers(0, 2, n * K).astype(np.uint32) << 31)).view(np.float32)
	fixed = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, np.float32(1.0) + np.float32(2.0 ** -8), 1.0, -511.0, 2.0 ** -126, 2.0 ** -149],
					 dtype=np.float32)
	kind = rng.integers(0, 4, n * K)
	x = np.where(kind == 1, sub, x)
	x = np.where(kind == 2, tie, x)
	x = np.where(kind == 3, fixed[rng.integers(0, fixed.size, n * K)], x)
	if n * K >= fixed.size:
		x[rng.permutation(n * K)[:fixed.size]] = fixed   # every fixed value at least once
	return x.reshape(n, K)


# ------------------------------------------------------------------ test 1: the pack kernel
@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("row_multiple", [1, 32])
@pytest.mark.parametrize("n,K", [(1, 1), (33, 7), (70, 85), (40, 170), (35, 256)])
def test_pack_split_bit_exact_on_poisoned_destination(ops, n, K, row_multiple, role):
	x = _special_values(n, K, seed=1000 * n + K)
	Kp = ops.split_kp(K)
	n_pad = -(-n // row_multiple) * row_multiple
	hi, lo = _split_bits(x)
	if n * K > 100:
		assert (lo != 0).any() and ((hi & 0x7f80) == 0x7f80).any() and np.isnan(x).any()   # the data does what the case is about
	want = _pack_split_np(hi, lo, role, Kp, n_pad)
	out = torch.full((n_pad, Kp), float("nan"), dtype=torch.bfloat16, device="cuda")
	got = ops.pack_split_bf16(torch.from_numpy(x).cuda(), role, Kp, row_multiple=row_multiple, out=out)
	assert got.data_ptr() == out.data_ptr()
	assert np.array_equal(_bits(got), want)   # segments, pad columns, pad rows
	# a source with a row pitch (a column slice of a wider matrix), default Kp, fresh destination
	wide = torch.full((n, K + 3), float("nan"), dtype=torch.float32, device="cuda")
	wide[:, 1:K + 1] = torch.from_numpy(x).cuda()
	assert np.array_equal(_bits(ops.pack_split_bf16(wide[:, 1:K + 1], role, row_multiple=row_multiple)), want)


@pytest.mark.parametrize("role", [0, 1])
def test_pack_split_bf16_input_has_zero_lo(ops, role):
	n, K = 37, 70
	x = torch.from_numpy(_special_values(n, K, seed=5)).bfloat16().cuda()
	hi = _bits(x)
	out = torch.full((64, ops.split_kp(K)), float("nan"), dtype=torch.bfloat16, device="cuda")
	got = _bits(ops.pack_split_bf16(x, role, row_multiple=32, out=out))
	assert np.array_equal(got, _pack_split_np(hi, np.zeros_like(hi), role, ops.split_kp(K), 64))


# ------------------------------------------------------------------ test 2: the rescore kernel alone
RS_Q, RS_I = 37, 1000


def _topk_by_score_then_id(scores, ids, valid, k):
	"""Per row: the k best valid (score, id) pairs, score descending, ties by the smaller id; (-inf, -1) padding.  float64 / int64 numpy."""
	Q = scores.shape[0]
	val = np.full((Q, k), -np.inf)
	idx = np.full((Q, k), -1, dtype=np.int64)
	for q in range(Q):
		j = np.nonzero(valid[q])[0]
		j = j[np.lexsort((ids[q, j], -scores[q, j]))][:k]
		val[q, :j.size], idx[q, :j.size] = scores[q, j], ids[q, j]
	return val, idx


def _candidates(rng, n_cand):
	return np.stack([rng.permutation(RS_I)[:n_cand] for _ in range(RS_Q)]).astype(np.int32)


@pytest.mark.parametrize("n_cand", [20, 130])
@pytest.mark.parametrize("K,pitch", [(1, 1), (70, 70), (70, 72), (256, 256)])   # pitch 70: rows not 16-byte aligned (element loads); 72: vector loads + a tail
def test_rescore_values_bit_equal_to_dense_gemm(ops, K, pitch, n_cand):
	g = torch.Generator().manual_seed(K * 1000 + n_cand)
	X = torch.randn(RS_Q, K, generator=g).cuda()
	Et = torch.full((RS_I, pitch), float("nan"), device="cuda")[:, :K]
	Et.copy_(torch.randn(RS_I, K, generator=g))
	cand = _candidates(np.random.default_rng(K + n_cand), n_cand)
	S = ops.gemm(X, Et.t()).cpu().numpy()                      # the dense fp32 route's scores
	sc = np.take_along_axis(S, cand.astype(np.int64), 1)
	for k_out in (1, 20, n_cand):
		want_v, want_i = _topk_by_score_then_id(sc.astype(np.float64), cand.astype(np.int64), np.ones_like(cand, dtype=bool), k_out)
		got = ops.rescore_topk(X, Et, torch.from_numpy(cand).cuda(), k_out)
		assert np.array_equal(got.indices.cpu().numpy(), want_i), (K, n_cand, k_out)
		assert np.array_equal(got.values.cpu().numpy().view(np.int32), want_v.astype(np.float32).view(np.int32)), (K, n_cand, k_out)
	# bf16 operands: the same chain on the up-converted values
	Xb, Eb = X.bfloat16(), Et.bfloat16()
	Sb = ops.gemm(Xb, Eb.t()).cpu().numpy()
	want_v, want_i = _topk_by_score_then_id(np.take_along_axis(Sb, cand.astype(np.int64), 1).astype(np.float64), cand.astype(np.int64),
											np.ones_like(cand, dtype=bool), 20)
	got = ops.rescore_topk(Xb, Eb, torch.from_numpy(cand).cuda(), 20)
	assert np.array_equal(got.indices.cpu().numpy(), want_i)
	assert np.array_equal(got.values.cpu().numpy().view(np.int32), want_v.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("n_cand", [20, 130])
@pytest.mark.parametrize("K", [1, 70, 256])
def test_rescore_ties_holes_padding_and_nan(ops, K, n_cand):
	"""Integer operands in {-1, 0, 1}: scores are small integers, ties everywhere -> order by the smaller id.  Holes (-1, >= I) are
	skipped, rows short of k_out valid candidates are padded with (-inf, -1), the candidate rows sit in a wider array (ld_idx > n_cand),
	and an item whose embedding holds a NaN is never selected."""
	rng = np.random.default_rng(7 * K + n_cand)
	Xn = rng.integers(-1, 2, (RS_Q, K)).astype(np.float32)
	En = rng.integers(-1, 2, (RS_I, K)).astype(np.float32)
	nan_items = rng.permutation(RS_I)[:100]
	cand = _candidates(rng, n_cand)
	holes = rng.random(cand.shape) < 0.15
	cand[holes] = np.where(rng.random(holes.sum()) < 0.5, -1, RS_I + rng.integers(0, 5, holes.sum()))
	cand[0, 3:] = -1          # three candidates left
	cand[1, :] = RS_I         # none left
	cand[2, 1:] = -1          # one
	wide = torch.full((RS_Q, n_cand + 5), 3, dtype=torch.int32, device="cuda")   # (3 is a valid id: reading past n_cand would show up as a duplicate)
	wide[:, :n_cand] = torch.from_numpy(cand).cuda()
	Et = torch.from_numpy(En).cuda()
	Et[torch.from_numpy(nan_items).cuda(), K // 2] = float("nan")
	S = Xn.astype(np.int64) @ En.astype(np.int64).T
	in_range = (cand >= 0) & (cand < RS_I)
	safe = np.where(in_range, cand, 0).astype(np.int64)
	valid = in_range & ~np.isin(safe, nan_items)
	assert (valid.sum(1) >= n_cand // 2).sum() > RS_Q // 2 and (~valid).sum() > RS_Q
	sc = np.take_along_axis(S, safe, 1).astype(np.float64)
	for k_out in (1, 20, n_cand):
		want_v, want_i = _topk_by_score_then_id(sc, cand.astype(np.int64), valid, k_out)
		got = ops.rescore_topk(torch.from_numpy(Xn).cuda(), Et, wide[:, :n_cand], k_out)
		assert np.array_equal(got.indices.cpu().numpy(), want_i), (K, n_cand, k_out)
		assert np.array_equal(got.values.cpu().numpy().astype(np.float64), want_v), (K, n_cand, k_out)


# ------------------------------------------------------------------ test 3: the sweep on split operands, exact data
def _reference(S, k):
	"""THE top-k of integer scores S [Q x I] (int64, CPU): (values, rows), values descending, ties by ascending row."""
	I = S.shape[1]
	assert I < 1 << 27 and int(S.abs().max()) < 1 << 24
	key = S * (1 << 27) - torch.arange(I, dtype=torch.int64)   # one key per (score, row): larger score first, then smaller row
	rows = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows), rows


@functools.lru_cache(maxsize=None)
def _exact_case(K):
	"""Integer operands with all three segments live and lo_x lo_e = 0 at every k: even k -- x odd in +-511 (9 significant bits: needs
	lo), e in +-15 (exact in bf16) --, odd k the reverse.  |S| <= 256 * 511 * 15 < 2^24: hi.hi + hi.lo + lo.hi is the integer X.E^T."""
	rng = np.random.default_rng(K)
	Q, I = 256, N_ITEMS
	def wide(shape):
		return (2 * rng.integers(0, 256, shape) + 1) * rng.choice([-1, 1], shape)
	def narrow(shape):
		return rng.integers(-15, 16, shape)
	even = (np.arange(K) % 2 == 0)[None, :]
	X = np.where(even, wide((Q, K)), narrow((Q, K))).astype(np.float32)
	E = np.where(even, narrow((I, K)), wide((I, K))).astype(np.float32)
	S = torch.from_numpy((X.astype(np.float64) @ E.astype(np.float64).T)).to(torch.int64)
	return torch.from_numpy(X), torch.from_numpy(E), S


@pytest.mark.parametrize("k", [10, 130])
@pytest.mark.parametrize("Q", [33, 256])
@pytest.mark.parametrize("K,Kp", [(70, 256), (150, 512), (256, 768)])
def test_split_sweep_exact_integer_data(ops, K, Kp, Q, k):
	I = N_ITEMS
	X, E, S = _exact_case(K)
	X, S = X[:Q], S[:Q]
	assert ops.split_kp(K) == Kp and ops.fused_supported(Q, I, Kp, k)
	if Kp > 512:
		assert ops.fused_plan(Q, I, Kp, k)["lg"] == 4   # the wide kernel
	Xp = ops.pack_split_bf16(X.cuda(), 0, Kp)
	Etp = ops.pack_split_bf16(E.cuda(), 1, Kp, row_multiple=32)
	lo_x, lo_e = Xp[:, :K].float().cpu(), Etp[:I, K:2 * K].float().cpu()
	assert (lo_x != 0).any() and (lo_e != 0).any() and not ((lo_x != 0) & (lo_e[:Q] != 0)).any()   # both cross terms live, lo.lo = 0
	got = ops.score_topk_fused(Xp, Etp, I, k)
	want_v, want_i = _reference(S, k + 1)
	assert torch.equal(got.values.cpu().to(torch.int64), want_v[:, :k])
	assert torch.equal(got.values.cpu(), want_v[:, :k].float())
	clear = (want_v[:, k - 1] != want_v[:, k]).numpy()
	assert clear.sum() > Q // 2
	gi, wi = np.sort(got.indices.cpu().numpy(), 1), np.sort(want_i[:, :k].numpy(), 1)
	assert np.array_equal(gi[clear], wi[clear])
	# without the lo segments the result is another one: the cross terms are exercised
	Xp0, Etp0 = Xp.clone(), Etp.clone()
	Xp0[:, :K] = 0
	Etp0[:, K:2 * K] = 0
	assert not torch.equal(ops.score_topk_fused(Xp0, Etp0, I, k).values.cpu(), want_v[:, :k].float())


# ------------------------------------------------------------------ test 4: the whole route on float data
ROUTE_Q, ROUTE_K = 100, 3       # k = 3: the bound is ~3e-4 of a score, the gap below rank k of 9371 items must clear it twice (condition (c))
ROUTE_K_LARGE = 100             # one-sided check at a realistic k (see test)
ROUTE_SEEDS = {64: 3, 256: 1}   # seeds whose fp64 scores put at most 2 % of the queries inside the gap (asserted below)


def _bound_coeff(K):
	return 2.0 ** -16 + 3 * K * 2.0 ** -23


def _gap_excused(S, tol, k):
	"""Per query: the k-th and (k+1)-th largest of S differ by no more than twice the tolerance at those elements."""
	o = np.argsort(-S, axis=1, kind="stable")[:, :k + 1]
	v, t = np.take_along_axis(S, o, 1), np.take_along_axis(tol, o, 1)
	return (v[:, k - 1] - v[:, k]) <= 2 * np.maximum(t[:, k - 1], t[:, k])


@functools.lru_cache(maxsize=None)
def _route_case(Ki):
	"""Protocol-B synthetic (rank 64, noise 0.05, Kq = 2 Ki): the two indexes, the queries, the dense fp32 scores, the fp64 scores and
	the elementwise tolerance.  Computed once per Ki and shared."""
	from anncur_amd import ops
	from anncur_amd.cur import CURRowIndex
	from oracle import cur_oracle as O
	seed = ROUTE_SEEDS[Ki]
	A_train, A_test = O.synth_protocol_b(2 * Ki, ROUTE_Q, N_ITEMS, rank=64, noise=0.05, seed=seed)
	anc = np.sort(np.random.default_rng(seed).choice(N_ITEMS, Ki, replace=False))
	R = A_train.cuda()
	A = torch.full((ROUTE_Q, N_ITEMS + 1), float("nan"), device="cuda")[:, :N_ITEMS]   # row pitch a multiple of 4 floats: what the packed error kernel takes
	A.copy_(A_test)
	dense = CURRowIndex(R, anc, compute_dtype="fp32", pinv_backend="numpy")
	split = CURRowIndex(R, anc, compute_dtype="bf16x3", pinv_backend="numpy")
	assert torch.equal(dense._Et, split._Et)
	X = ops.gather_cols(A, anc)
	S32 = ops.gemm(X, dense._Et.t()).cpu().numpy()
	X64, E64 = X.cpu().double().numpy(), dense._Et.cpu().double().numpy()
	S64 = X64 @ E64.T
	tol = _bound_coeff(Ki) * (np.abs(X64) @ np.abs(E64).T)
	return dict(dense=dense, split=split, X=X, A=A, S32=S32, S64=S64, tol=tol)


@pytest.mark.parametrize("Ki", [64, 256])
def test_route_cur_row_index_matches_dense_fp32(ops, Ki):
	c = _route_case(Ki)
	k, Q, I = ROUTE_K, ROUTE_Q, N_ITEMS
	Kp = ops.split_kp(Ki)
	assert Kp == (256 if Ki == 64 else 768)
	assert ops.fused_supported(Q, I, Kp, ops.split_candidates(I, k)) and c["split"]._split.takes(Q, I, k)
	# (c) the condition on the data, from fp64 alone: at most 2 % of the queries inside the gap
	assert _gap_excused(c["S64"], c["tol"], k).mean() <= 0.02
	want = c["dense"].topk(c["X"], k)
	got = c["split"].topk(c["X"], k)
	gi, gv = got.indices.cpu().numpy().astype(np.int64), got.values.cpu().numpy()
	# (a) values bit-equal to the dense fp32 route's for the same (q, item), descending
	assert np.array_equal(gv.view(np.int32), np.take_along_axis(c["S32"], gi, 1).view(np.int32))
	assert (np.diff(gv, axis=1) <= 0).all()
	# (b) same sets wherever the dense route's k-th and (k+1)-th scores are more than twice the tolerance apart
	excused = _gap_excused(c["S32"].astype(np.float64), c["tol"], k)
	assert excused.mean() <= 0.02
	wi = want.indices.cpu().numpy().astype(np.int64)
	assert np.array_equal(np.sort(gi, 1)[~excused], np.sort(wi, 1)[~excused])
	# a realistic k, one-sided (most queries have SOME near-tie at rank 100, so set equality is no condition there): every item that
	# clears the (k+1)-th score by more than twice the tolerance is returned, with the dense value; nothing below the k-th by as much is
	kl = ROUTE_K_LARGE
	assert c["split"]._split.takes(Q, I, kl)
	got = c["split"].topk(c["X"], kl)
	gi, gv = got.indices.cpu().numpy().astype(np.int64), got.values.cpu().numpy()
	assert np.array_equal(gv.view(np.int32), np.take_along_axis(c["S32"], gi, 1).view(np.int32)) and (np.diff(gv, axis=1) <= 0).all()
	srt = -np.sort(-c["S64"], axis=1)
	margin = 2 * c["tol"].max(axis=1)
	for q in range(Q):
		must = np.nonzero(c["S64"][q] > srt[q, kl] + margin[q])[0]
		assert np.isin(must, gi[q]).all(), q
		assert (c["S64"][q, gi[q]] >= srt[q, kl - 1] - margin[q]).all(), q


@pytest.mark.parametrize("Ki", [64, 256])
def test_route_raw_split_scores_within_bound_and_bf16_outside(ops, Ki):
	"""(d) the sweep's own scores on the split operands (no rescore) against fp64, element by element; the plain bf16 operands miss the
	same bound on the same data: the bound discriminates."""
	c = _route_case(Ki)
	k, I = 50, N_ITEMS
	Et, X = c["dense"]._Et, c["X"]
	Kp = ops.split_kp(Ki)
	assert ops.fused_supported(ROUTE_Q, I, Kp, k)
	raw = ops.score_topk_fused(ops.pack_split_bf16(X, 0, Kp), ops.pack_split_bf16(Et, 1, Kp, row_multiple=32), I, k)
	ri = raw.indices.cpu().numpy().astype(np.int64)
	err = np.abs(raw.values.cpu().numpy().astype(np.float64) - np.take_along_axis(c["S64"], ri, 1))
	lim = np.take_along_axis(c["tol"], ri, 1)
	print(f"Ki={Ki}: split max err / bound = {(err / lim).max():.3f}")
	assert (err <= lim).all()
	Kp16 = ops.padded_k(Ki)
	b = ops.score_topk_fused(ops.pack_bf16(X, Kp16), ops.pack_bf16(Et, Kp16, row_multiple=32), I, k)
	bi = b.indices.cpu().numpy().astype(np.int64)
	errb = np.abs(b.values.cpu().numpy().astype(np.float64) - np.take_along_axis(c["S64"], bi, 1))
	print(f"Ki={Ki}: bf16 max err / bound = {(errb / np.take_along_axis(c['tol'], bi, 1)).max():.1f}")
	assert (errb > np.take_along_axis(c["tol"], bi, 1)).any()


@pytest.mark.parametrize("Ki", [64, 256])
def test_route_approx_error_rows_within_1e4_of_fp32(ops, Ki):
	"""(e) Ki = 64: the packed error kernel on the split operands (Kp = 256); Ki = 256: Kp = 768, the fp32 kernel as before."""
	c = _route_case(Ki)
	assert ops.approx_error_packed_ok(ops.split_kp(Ki), c["A"]) == (Ki == 64)
	err, nrm = c["split"].approx_error_rows(c["X"], c["A"])
	err32, nrm32 = ops.approx_error(c["X"], c["dense"]._Et, c["A"])
	e, e32 = err.double().cpu().numpy(), err32.double().cpu().numpy()
	print(f"Ki={Ki}: max relative difference of the per-row error sums = {(np.abs(e - e32) / e32).max():.2e}")
	assert (np.abs(e - e32) <= 1e-4 * e32).all()
	# sum A^2: the same 9371 fp32 squares summed in fp32 by two kernels in two orders.  Each sum is only good to (n - 1) 2^-24 ~ 5.6e-4
	# relative in the worst case and ~sqrt(n) 2^-24 ~ 6e-6 typically, so they cannot be asked to agree to the last bits; the bar is the
	# one this call is held to for the error sums, 1e-4 relative.
	n, n32 = nrm.double().cpu().numpy(), nrm32.double().cpu().numpy()
	print(f"Ki={Ki}: max relative difference of the per-row norm sums = {(np.abs(n - n32) / n32).max():.2e}")
	assert (np.abs(n - n32) <= 1e-4 * n32).all()


FLAT_D, FLAT_NQ, FLAT_K, FLAT_SEED = 96, 100, 5, 1   # seed: no query of the 100 inside the gap in fp64 (asserted in the test)


def test_route_flat_ip_index_matches_fp32(ops):
	from anncur_amd.nearest_nbr import FlatIPIndex
	rng = np.random.default_rng(FLAT_SEED)
	Xv = rng.standard_normal((N_ITEMS, FLAT_D)).astype(np.float32)
	q = rng.standard_normal((FLAT_NQ, FLAT_D)).astype(np.float32)
	Kp = ops.split_kp(FLAT_D)
	assert Kp == 512 and ops.fused_supported(FLAT_NQ, N_ITEMS, Kp, ops.split_candidates(N_ITEMS, FLAT_K))
	S64 = q.astype(np.float64) @ Xv.astype(np.float64).T
	tol = _bound_coeff(FLAT_D) * (np.abs(q).astype(np.float64) @ np.abs(Xv).astype(np.float64).T)
	assert _gap_excused(S64, tol, FLAT_K).mean() <= 0.02
	a, b = FlatIPIndex(FLAT_D, dtype="fp32"), FlatIPIndex(FLAT_D, dtype="bf16x3")
	a.add(Xv); b.add(Xv)
	Da, Ia = a.search(q, FLAT_K)
	Db, Ib = b.search(q, FLAT_K)
	assert b._split is not None and b._split.takes(FLAT_NQ, N_ITEMS, FLAT_K)
	S32 = ops.gemm(torch.from_numpy(q).cuda(), torch.from_numpy(Xv).cuda().t()).cpu().numpy()
	assert Db.dtype == np.float32 and Ib.dtype == np.int64
	assert np.array_equal(Db.view(np.int32), np.take_along_axis(S32, Ib, 1).view(np.int32))
	excused = _gap_excused(S32.astype(np.float64), tol, FLAT_K)
	assert excused.mean() <= 0.02
	assert np.array_equal(np.sort(Ia, 1)[~excused], np.sort(Ib, 1)[~excused])
	# a tiny index (outside the fused path: the dense route serves it) asked for more results than it stores: FAISS padding as on the other routes
	c = FlatIPIndex(FLAT_D, dtype="bf16x3")
	c.add(Xv[:50])
	D, I = c.search(q[:3], 64)
	assert (I[:, 50:] == -1).all() and (np.sort(I[:, :50], 1) == np.arange(50)).all() and (D[:, 50:] == np.finfo(np.float32).min).all()


# ------------------------------------------------------------------ test 5: the entry points
def _dump(path, scores, **extra):
	os.makedirs(os.path.dirname(path), exist_ok=True)
	d = {"ment_to_ent_scores": scores, "ment_to_ent_scores.shape": tuple(scores.shape), "test_data": [], "mention_tokens_list": [[0] * 4] * scores.shape[0],
		 "entity_id_list": np.arange(scores.shape[1]), "entity_tokens_list": [], "arg_dict": {}}
	d.update(extra)
	with open(path, "wb") as f:
		pickle.dump(d, f)


def _assert_same_metrics(got, want, n_queries, top_k, where):
	"""The bf16x3 run against the default (fp32) run of the same CLI: the reference's 4 decimals, plus ONE swapped boundary near-tie
	(one count in one query -- 1 / n on a count mean, 1 / (n top_k) on a fraction mean, one count on a median)."""
	assert set(got) == set(want), where
	for m, w in want.items():
		g = got[m]
		if isinstance(w, float) and np.isnan(w):
			assert np.isnan(g), (where, m)
			continue
		frac = "_frac_" in m
		one = (1.0 / top_k) if frac else 1.0
		if m.startswith("approx_error"):
			assert g == pytest.approx(w, rel=1e-4), (where, m, g, w)
		elif m.endswith("_p50"):
			assert abs(g - w) <= one + 1e-9, (where, m, g, w)
		elif m.endswith("_std"):
			assert abs(g - w) <= 1e-3 * (1.0 if frac else top_k) + one / max(n_queries, 1) ** 0.5, (where, m, g, w)
		else:
			assert abs(g - w) <= 1.0001e-4 * (1.0 if frac else top_k) + one / max(n_queries, 1), (where, m, g, w)


def test_entry_point_A_cli_bf16x3_reproduces_default_json(ops, tmp_path, golden_meta):
	"""golden_meta["entryA"]["input"] (1000 x 5000 fp32, 64 anchors).  5000 items are below the fused path's minimum, so the retrieval
	of this cell falls back to the dense route, as the issue of an unsupported shape must; the error sums run on the split operands."""
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from utils.zeshel_utils import score_matrix_filename
	torch.manual_seed(0)
	A = torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)
	res = {}
	for tag, extra in (("fp32", []), ("x3", ["--compute_dtype", "bf16x3"])):
		res_dir = str(tmp_path / tag)
		_dump(score_matrix_filename(res_dir, "yugioh", 1000), A)
		out_dir = epA.main(["--data_name", "yugioh", "--res_dir", res_dir, "--n_ment", "1000", "--n_seeds", "2", "--disable_wandb", "1", "--misc", tag,
							"--eval_methods", "cur,cur_oracle", "--n_ment_anchors_vals", "128", "--n_ent_anchors_vals", "64",
							"--top_k_vals", "10", "--top_k_retr_vals", "100", "--pinv", "numpy"] + extra)
		with open(os.path.join(out_dir, "retrieval_wrt_exact_crossenc.json")) as f:
			res[tag] = json.load(f)
	assert res["x3"]["other_args"]["arg_dict"]["compute_dtype"] == "bf16x3" and res["fp32"]["other_args"]["arg_dict"]["compute_dtype"] == "auto"
	assert set(res["x3"]) == set(res["fp32"]) == {"cur", "cur_oracle", "other_args"}
	sizes = {"anchor": 128, "non_anchor": 872, "all": 1000}
	for method in ("cur", "cur_oracle"):
		a, b = (res[t][method]["top_k=10"]["k_retvr=100"]["anc_n_m=128~anc_n_e=64"] for t in ("fp32", "x3"))
		for t, n in sizes.items():
			_assert_same_metrics(b[t], a[t], n, 10, (method, t))
	gold = golden_meta["entryA"]["results"]["cur_kq128_ki64_2seeds"]["all"]
	key = "exact_vs_reranked_approx_retvr~common_frac_mean"
	assert res["x3"]["cur"]["top_k=10"]["k_retvr=100"]["anc_n_m=128~anc_n_e=64"]["all"][key] == pytest.approx(gold[key], abs=1.0001e-4 + 1e-4)


def test_entry_point_B_cli_bf16x3_reproduces_default_json(ops, tmp_path, golden_meta):
	"""golden_meta["entryB"]["input"] (500 train / 2000 test x 20000, 256 anchors: Kp = 768, the wide kernel, inside the fused path) and
	golden_meta["entryB_sweep"]["input"] (600 items: every cell falls back to the dense route)."""
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	from oracle import cur_oracle as O
	assert ops.fused_supported(2000, 20000, ops.split_kp(256), ops.split_candidates(20000, 100))
	A_train, A_test = O.synth_protocol_b(500, 2000, 20000, rank=64, noise=0.05, seed=0)
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	S_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	S_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	cases = {"big": (A_train, A_test, ["--top_k_vals", "1,10,100", "--top_k_retr_vals", "100", "--n_ent_anchors_vals", "256"]),
			 "small": (S_train, S_test, ["--top_k_vals", "1,10", "--top_k_retr_vals", "10,50", "--n_ent_anchors_vals", "10,30"])}
	for name, (tr, te, grid) in cases.items():
		_dump(str(tmp_path / name / "train.pkl"), tr, ment_idxs=list(range(tr.shape[0])))
		_dump(str(tmp_path / name / "test.pkl"), te, ment_idxs=list(range(tr.shape[0], tr.shape[0] + te.shape[0])))
		res = {}
		for tag, extra in (("fp32", []), ("x3", ["--compute_dtype", "bf16x3"])):
			f = epB.main(["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / name / "out"), "--test_data_file", str(tmp_path / name / "test.pkl"),
						  "--train_data_file", str(tmp_path / name / "train.pkl"), "--n_seeds", "1", "--misc", tag, "--pinv", "numpy"] + grid + extra)
			with open(f) as fh:
				res[tag] = json.load(fh)
		assert res["x3"]["other_args"]["compute_dtype"] == "bf16x3"
		a, b = res["fp32"]["seed=0"], res["x3"]["seed=0"]
		assert set(a) == set(b)
		n_cells = 0
		for tk in a:
			for kr in a[tk]:
				assert set(a[tk][kr]) == set(b[tk][kr])
				for cell in a[tk][kr]:
					_assert_same_metrics(b[tk][kr][cell], a[tk][kr][cell], te.shape[0], int(tk.split("=")[1]), (name, tk, kr, cell))
					n_cells += 1
		assert n_cells >= 3
		if name == "big":
			gold = golden_meta["entryB"]["all_topk_kretvr100"]
			for k in (1, 10, 100):
				for m, v in gold[str(k)].items():
					if m.endswith("common_frac_mean"):
						assert b[f"top_k={k}"]["k_retvr=100"]["anc_n_m=500_anc_n_e=256"][m] == pytest.approx(v, abs=1.0001e-4 + 1.0 / (2000 * k)), (k, m)
