"""Subnormal scores and operands through the routes that are neither a strided GEMM nor a fused sweep: the ranks (ops.score_rank,
ops.rank_in_rows), the selectors that pass values through (ops.rerank, ops.rerank_scored, ops.filter_topk), the IVF scans, the sparse
inner-product route and the fp64 gather of ops.lstsq_rows.

References: tests/subnormal_cases.py (integers times a power of two: every product and partial sum exact, in any order), tests/rank_numpy.py,
tests/topk_numpy.py, tests/sparse_numpy.py.  All on the host, held there by tests/test_cpu_subnormal_reference.py and the references' own CPU
tests; nothing is read back from the device to form an expectation; every comparison is on integer views or integer results, without a
tolerance.  A device that read a subnormal as zero would tie it with the zeros of its row (ranks and ids change), return zero scores
(sub-in), or lose the item; each test says in its docstring where it would show.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_numpy as rn  # noqa: E402
import sparse_numpy as sp  # noqa: E402
import subnormal_cases as sn  # noqa: E402
import test_gpu_fused_nonfinite as tn  # noqa: E402  (its operand helper; pytest collects none of its tests from here)
from topk_numpy import rerank_ref  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _eq_bits(got, want, what):
	g, w = sn.bits32(np.ascontiguousarray(got)), sn.bits32(np.ascontiguousarray(want))
	assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {w.size} values differ in their bits (all zero on the device: {not np.asarray(got).any()})"


# ------------------------------------------------------------------ 6. ranks
def _target_ids(rng, Q, I, t):
	ids = np.stack([rng.permutation(I)[:t] for _ in range(Q)]).astype(np.int32)
	ids[rng.random(ids.shape) < 0.1] = -1                       # holes
	ids[:, 1] = ids[:, 0]                                       # a duplicate
	return ids


@pytest.mark.parametrize("name", ["all-sub", "sub-in"])
@pytest.mark.parametrize("Kp", [64, 512])
def test_score_rank_on_subnormal_scores_and_operands(ops, Kp, name):
	"""all-sub: every score n 2^-149 -- a flushed score ties the whole row at zero and every rank becomes the id order; sub-in: flushed
	operands do the same.  Ranks against rank_numpy.rank_ref on the host scores, the score output bit for bit (NaN at a hole)."""
	Q, I, t = 70, 4101, 100
	case = sn.IntCase(name, Q, I, Kp - 9, seed=Kp)
	ids = _target_ids(np.random.default_rng(Kp), Q, I, t)
	want = rn.rank_ref(case.S, ids)
	zero = rn.rank_ref(np.zeros_like(case.S), ids)
	assert (want != zero).mean() > 0.8                            # the ranks of an all-tied row are far from the true ones
	Xp, Etp = tn._operands(case, Kp)
	assert ops.score_rank_ok(Kp, I, t)
	rank, score = ops.score_rank(Xp, Etp, I, torch.from_numpy(ids), return_scores=True)
	torch.cuda.synchronize()
	got_s = score.cpu().numpy()
	hole = ids < 0
	assert np.isnan(got_s[hole]).all()
	_eq_bits(got_s[~hole], np.take_along_axis(case.values32(), np.maximum(ids, 0).astype(np.int64), 1)[~hole], f"score_rank Kp={Kp} {name}: scores")
	got_r = rank.cpu().numpy()
	assert np.array_equal(got_r, want), f"score_rank Kp={Kp} {name}: {int((got_r != want).sum())} of {want.size} ranks differ (equal to the ranks of an all-zero row: {np.array_equal(got_r, zero)})"


def _mixed_row_bits(rng, Q, I, bf16):
	"""Rows of subnormals of both signs (fp32: n 2^-149, |n| <= 40; bf16: m 2^-133, |m| <= 40: tie-heavy), +0, -0, and normal numbers of both signs
	down to +-2^-126 -> uint32 patterns [Q x I] (bf16: the pattern in the upper half, the lower half zero)."""
	n = rng.integers(-40, 41, (Q, I))
	shift = 16 if bf16 else 0
	u = (np.abs(n).astype(np.uint32) << shift) | np.where(n < 0, np.uint32(0x80000000), np.uint32(0))
	kind = rng.random((Q, I))
	u = np.where(kind < 0.05, np.uint32(0), u)                                    # +0
	u = np.where((kind >= 0.05) & (kind < 0.10), np.uint32(0x80000000), u)        # -0
	normal = (np.uint32(0x00800000) + (rng.integers(0, 4, (Q, I)).astype(np.uint32) << 16)) | np.where(rng.random((Q, I)) < 0.5, np.uint32(0x80000000), np.uint32(0))
	u = np.where((kind >= 0.10) & (kind < 0.15), normal, u)                       # +-2^-126 (1 + j / 128), j = 0, 2, 4, 6
	u = np.where((kind >= 0.15) & (kind < 0.17), np.where(n < 0, np.uint32(0xbf800000), np.uint32(0x3f800000)), u)   # +-1
	return u


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_rank_in_rows_ties_only_the_two_zeros(ops, bf16):
	"""rank_in_rows folds -0 onto +0 with `v == 0.0f`: that compare must be true for the two zeros only.  Rows with an odd pitch inside a NaN-filled
	buffer, t = 64 targets among them zeros of both signs, the smallest subnormals of both signs and holes.  A subnormal read as zero changes
	the rank of every zero and of every subnormal."""
	Q, I, t = 9, 4101, 64
	rng = np.random.default_rng(17 + bf16)
	u = _mixed_row_bits(rng, Q, I, bf16)
	S32 = u.view(np.float32)
	sub = sn.is_subnormal(S32)
	assert sub.mean() > 0.7 and (u == 0).any(1).all() and (u == 0x80000000).any(1).all() and (~sub & (S32 != 0)).any(1).all()
	ids = _target_ids(rng, Q, I, t)
	for q in range(Q):      # targets of every kind in every row
		for j, pick in enumerate((u[q] == 0, u[q] == 0x80000000, S32[q] == np.float32(2.0 ** -133), S32[q] == np.float32(-2.0 ** -133), S32[q] == np.float32(2.0 ** -126))):
			ids[q, 2 + j] = np.flatnonzero(pick)[q % max(1, np.count_nonzero(pick))] if pick.any() else ids[q, 2 + j]
	want = rn.rank_ref(S32, ids)
	flushed = rn.rank_ref(sn.flush(S32), ids)
	assert (want != flushed).mean() > 0.5
	dt = BF16 if bf16 else F32
	buf = torch.full((Q + 2, I + 4), float("nan"), dtype=dt, device="cuda")
	S = buf[1:Q + 1, 1:I + 1]
	host = torch.from_numpy((u >> 16).astype(np.uint16).view(np.int16)).view(BF16) if bf16 else torch.from_numpy(S32.copy())
	S.copy_(host)
	assert S.stride(0) % 2 == 1
	back = S.cpu()
	assert np.array_equal(back.view(torch.int16 if bf16 else torch.int32).numpy(), host.view(torch.int16 if bf16 else torch.int32).numpy())   # the copy kept every pattern
	rank, score = ops.rank_in_rows(S, torch.from_numpy(ids), return_scores=True)
	torch.cuda.synchronize()
	hole = ids < 0
	got_s = score.cpu().numpy()
	assert np.isnan(got_s[hole]).all()
	_eq_bits(got_s[~hole], np.take_along_axis(S32, np.maximum(ids, 0).astype(np.int64), 1)[~hole], "rank_in_rows: scores")
	got_r = rank.cpu().numpy()
	assert np.array_equal(got_r, want), f"{int((got_r != want).sum())} of {want.size} ranks differ (equal to the ranks of the flushed rows: {np.array_equal(got_r, flushed)})"


# ------------------------------------------------------------------ 7. selectors that pass values through
def _all_subnormal_rows(rng, Q, I, bf16):
	"""[Q x I] float32 values, every one a subnormal (fp32: n 2^-149, 1 <= |n| <= 300; bf16: m 2^-133, 1 <= |m| <= 127): tie-heavy, both signs."""
	hi = 127 if bf16 else 300
	n = rng.integers(1, hi + 1, (Q, I)) * (2 * rng.integers(0, 2, (Q, I)) - 1)
	v = (n * (sn.BF16_STEP if bf16 else sn.F32_STEP)).astype(np.float32)
	assert sn.is_subnormal(v).all()
	return v


def _device_rows(v, bf16):
	Q, I = v.shape
	buf = torch.full((Q + 2, I + 8), float("nan"), dtype=BF16 if bf16 else F32, device="cuda")
	A = buf[1:Q + 1, 3:I + 3]
	A.copy_(sn.to_bf16_exact(v) if bf16 else torch.from_numpy(v))
	return A


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k_retvr,k_out", [(130, 100), (520, 200), (700, 600)])
def test_rerank_on_all_subnormal_rows(ops, k_retvr, k_out, bf16):
	"""ops.rerank: the k_out best of k_retvr given items by exact score, value descending then id: every score a subnormal, so a flush
	orders every row by id alone."""
	Q, I = 9, 4101
	rng = np.random.default_rng([k_retvr, k_out, int(bf16)])
	v = _all_subnormal_rows(rng, Q, I, bf16)
	cand = np.stack([rng.permutation(I)[:k_retvr] for _ in range(Q)]).astype(np.int32)
	want = [rerank_ref(v[q], cand[q], k_out) for q in range(Q)]
	want_v, want_i = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
	assert (want_i != np.sort(cand, axis=1)[:, :k_out]).mean() > 0.9
	got = ops.rerank(_device_rows(v, bf16), torch.from_numpy(cand).cuda(), k_retvr, k_out)
	torch.cuda.synchronize()
	_eq_bits(got.values.cpu().numpy(), want_v, f"rerank {k_retvr}->{k_out}")
	assert np.array_equal(got.indices.cpu().numpy(), want_i)


@pytest.mark.parametrize("sh_bf16", [False, True], ids=["shared-f32", "shared-bf16"])
@pytest.mark.parametrize("k", [100, 200, 600])
def test_rerank_scored_on_all_subnormal_scores(ops, k, sh_bf16):
	"""ops.rerank_scored: a pool of 300 shared ids (scores fp32 or bf16) and 700 per-query candidates (fp32), a tenth of them also shared (the
	shared score stands) and some holes; every score a subnormal."""
	Q, I, n_sh, n_pq = 9, 4101, 300, 700
	rng = np.random.default_rng([k, int(sh_bf16)])
	sh_ids = np.sort(rng.permutation(I)[:n_sh]).astype(np.int32)
	sh_val = _all_subnormal_rows(rng, Q, n_sh, sh_bf16)
	pq_val = _all_subnormal_rows(rng, Q, n_pq, False)
	pq_ids = np.stack([rng.permutation(I)[:n_pq] for _ in range(Q)]).astype(np.int32)
	pq_ids[:, :70] = np.stack([rng.permutation(sh_ids)[:70] for _ in range(Q)])
	pq_ids[rng.random(pq_ids.shape) < 0.03] = -1
	want_v, want_i = np.full((Q, k), -np.inf, dtype=np.float32), np.full((Q, k), -1, dtype=np.int64)
	for q in range(Q):
		keep = (pq_ids[q] >= 0) & ~np.isin(pq_ids[q], sh_ids)
		ids = np.concatenate([sh_ids, pq_ids[q][keep]]).astype(np.int64)
		val = np.concatenate([sh_val[q], pq_val[q][keep]])
		assert np.unique(ids).size == ids.size >= k
		order = np.lexsort((ids, -val.astype(np.float64)))[:k]
		want_v[q], want_i[q] = val[order], ids[order]
	got = ops.rerank_scored(k, cand=torch.from_numpy(pq_ids).cuda(), cand_scores=torch.from_numpy(pq_val).cuda(), shared_ids=sh_ids,
							shared_scores=_device_rows(sh_val, sh_bf16))
	torch.cuda.synchronize()
	_eq_bits(got.values.cpu().numpy(), want_v, f"rerank_scored k={k}")
	assert np.array_equal(got.indices.cpu().numpy().astype(np.int64), want_i)


@pytest.mark.parametrize("k_out", [100, 200, 600])
def test_filter_topk_passes_subnormal_values_through(ops, k_out):
	"""ops.filter_topk: a stable compaction of rows that are a top-k result (descending, ties by id), every value a subnormal."""
	Q, n_cand, I = 9, 800, 4101
	rng = np.random.default_rng(k_out)
	v = -np.sort(-_all_subnormal_rows(rng, Q, n_cand, False).astype(np.float64), axis=1).astype(np.float32)
	idx = np.stack([rng.permutation(I)[:n_cand] for _ in range(Q)]).astype(np.int32)
	idx[rng.random(idx.shape) < 0.05] = -1
	excl = [np.unique(rng.choice(idx[q][idx[q] >= 0], 60)) for q in range(Q)]
	want_v, want_i = np.full((Q, k_out), -np.inf, dtype=np.float32), np.full((Q, k_out), -1, dtype=np.int32)
	for q in range(Q):
		keep = np.flatnonzero((idx[q] >= 0) & ~np.isin(idx[q], excl[q]))[:k_out]
		want_v[q, :keep.size], want_i[q, :keep.size] = v[q, keep], idx[q, keep]
	got = ops.filter_topk(torch.from_numpy(v).cuda(), torch.from_numpy(idx).cuda(), excl, k_out)
	torch.cuda.synchronize()
	_eq_bits(got.values.cpu().numpy(), want_v, f"filter_topk k_out={k_out}")
	assert np.array_equal(got.indices.cpu().numpy(), want_i)


# ------------------------------------------------------------------ 9. the sparse route: two separately rounded steps per term
def _scaled(m, e):
	data = (m.data.astype(np.float64) * 2.0 ** e).astype(np.float32)
	assert (data.astype(np.float64) == m.data.astype(np.float64) * 2.0 ** e).all()
	return sp.CSR(m.indptr, m.indices, data, m.shape)


@pytest.mark.parametrize("name,eq,ei", [("all-sub", -70, -79), ("sub-in", -145, 122)])
def test_sparse_rows_and_topk(ops, name, eq, ei):
	"""ops.sparse_score_rows (S and the maxima of 64 consecutive items) and ops.sparse_score_topk.  all-sub: q_val = ints 2^-70, post_val = ints 2^-79:
	every product fl(w v) and every sum is n 2^-149, exact.  sub-in: q_val = ints 2^-145 (subnormal operands of the multiply), post_val = ints
	2^122: products n 2^-23.  The reference is sparse_numpy.scores_ref in float32 on the host, which must equal the integer product times 2^u."""
	Q, I, V, k = 5, 4101, 300, 100
	rng = np.random.default_rng([eq & 0xff, ei & 0xff])
	qi, it = sp.integer_csr(rng, Q, V, 40, 120), sp.integer_csr(rng, I, V, 5, 40)
	queries, items = _scaled(qi, eq), _scaled(it, ei)
	N = sp.densify(qi).astype(np.int64) @ sp.densify(it).astype(np.int64).T
	assert int((np.abs(sp.densify(qi)).astype(np.int64) @ np.abs(sp.densify(it)).astype(np.int64).T).max()) < 1 << 23
	want = (N.astype(np.float64) * 2.0 ** (eq + ei)).astype(np.float32)
	S = sp.scores_ref(queries, items)
	assert np.array_equal(S, want) and np.array_equal(np.abs(S), np.abs(want)) and (S != 0).mean() > 0.5    # (by value: a chain that ends at -0 + 0 is +0 either way)
	want = S
	if name == "all-sub":
		assert (sn.is_subnormal(want) | (want == 0)).all() and not sn.is_subnormal(queries.data).any() and not sn.is_subnormal(items.data).any()
	else:
		assert sn.is_subnormal(queries.data[queries.data != 0]).all() and not sn.is_subnormal(want).any()
	postings = ops.sparse_postings(*items.triple, I, V)
	got_S, got_GM = ops.sparse_score_rows(queries, postings)
	torch.cuda.synchronize()
	_eq_bits(got_S.cpu().numpy(), want, f"sparse {name}: S")
	_eq_bits(got_GM.cpu().numpy(), sp.group_maxima(want), f"sparse {name}: GM")
	ws = ops.sparse_workspace(Q, I, k, torch.device("cuda"))
	ws.fill_(0xff)
	got = ops.sparse_score_topk(queries, postings, k, workspace=ws)
	torch.cuda.synchronize()
	order = np.lexsort((np.broadcast_to(np.arange(I), want.shape), -want.astype(np.float64)), axis=-1)[:, :k]
	_eq_bits(got.values.cpu().numpy(), np.take_along_axis(want, order, 1), f"sparse {name}: top-k values")
	assert np.array_equal(got.indices.cpu().numpy().astype(np.int64), order), f"sparse {name}: ids"


# ------------------------------------------------------------------ 8. IVF: the hand-built lists of tests/test_gpu_ivf_exact.py, rescaled
IVF_SIZES = [64, 63, 65, 0, 70, 33, 66]        # nlist = 7, sizes around the 64-vector tile edge, one empty list


def _ivf_tensor(a, e, dtype, dev, pad):
	"""The integer matrix a times 2^e as the [:, :d] view of a row-padded tensor of `dtype` (exact, asserted); the padding holds 5."""
	v = a.astype(np.float64) * 2.0 ** e
	t = sn.to_bf16_exact(v) if dtype == BF16 else torch.from_numpy(v.astype(np.float32))
	assert (t.double().numpy() == v).all()
	buf = torch.full((a.shape[0], a.shape[1] + pad), 5.0, dtype=dtype)
	buf[:, :a.shape[1]] = t
	return buf.to(dev)[:, :a.shape[1]]


def _ivf_equal(got, want, u, what):
	wv = np.where(np.isinf(want[0]), want[0].astype(np.float64), want[0].astype(np.float64) * 2.0 ** u).astype(np.float32)
	gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy().astype(np.int32)
	assert np.array_equal(sn.bits32(gv), sn.bits32(wv)), f"{what}: {int((sn.bits32(gv) != sn.bits32(wv)).sum())} of {wv.size} values differ (every finite value zero on the device: {not gv[np.isfinite(gv)].any()})"
	assert np.array_equal(gi, want[1]), f"{what}: ids differ in {int((gi != want[1]).any(1).sum())} queries"


@pytest.mark.parametrize("name", ["all-sub", "sub-in"])
@pytest.mark.parametrize("dtype,dp", [(F32, 48), (BF16, 80), (BF16, 128)], ids=["fp32-64x64", "bf16-64x64", "bf16-tile128"])
def test_ivf_search_grouped_on_subnormal_scores_and_operands(ops, dtype, dp, name):
	"""ops.ivf_search_grouped on the three tile bodies.  all-sub: lists ints 2^-70, queries ints 2^-79: every score n 2^-149.  sub-in: the queries
	are subnormals (bf16: ints 2^-133; fp32: ints 2^-145), the lists ints 2^110 / 2^122: scores n 2^-23, zero for a body that reads subnormal
	operands as zero.  Values bit for bit, ids by the packed tie rule, on poisoned scratch."""
	import test_gpu_ivf_exact as iv
	from anncur_amd import _lib
	dev = torch.device("cuda")
	eq, ex = (-79, -70) if name == "all-sub" else ((-133, 110) if dtype == BF16 else (-145, 122))
	g = np.random.default_rng([dp, len(name)])
	sizes = np.asarray(IVF_SIZES, dtype=np.int64)
	nq, nprobe, k, vr = 70, 3, 64, (8 if name == "all-sub" else 4)
	probe = iv._random_probe(g, nq, nprobe, len(sizes), invalid=0.1)
	n = int(sizes.sum())
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X, Q = g.integers(-vr, vr + 1, (n, dp)).astype(np.int64), g.integers(-vr, vr + 1, (nq, dp)).astype(np.int64)
	assert vr * vr * dp < 1 << 23
	Xd, Qd = _ivf_tensor(X, ex, dtype, dev, 8), _ivf_tensor(Q, eq, dtype, dev, 16)
	if name == "sub-in":
		qv = Qd.float().cpu().numpy()
		assert sn.is_subnormal(qv[qv != 0]).all()
	want_tile = 128 if dtype == BF16 and dp % 128 == 0 else 64
	assert _lib.load().anncur_ivf_search_tile(ops._dt(Xd), dp, ops._ld(Xd), ops._ld(Qd), nq) == want_tile
	want = iv._reference(X, Q, off, ids, probe, k, ("packed",))["packed"]
	assert (want[0][np.isfinite(want[0])] != 0).mean() > 0.9
	off_d, ids_d, probe_d = torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(probe).to(dev)
	got = iv._poisoned(ops, lambda: ops.ivf_search_grouped(Xd, off_d, ids_d, sizes, Qd, probe_d, k))
	_ivf_equal(got, want, eq + ex, f"ivf_search_grouped tile{want_tile} {name}")


@pytest.mark.parametrize("name", ["all-sub", "sub-in"])
def test_ivf_scans_on_subnormal_scores_and_operands(ops, name):
	"""ops.ivf_scan (the per-query scan) and ops.ivf_scan_grouped with fp32 lists and with bf16 lists, on bf16-exact data in fp32 tensors
	(sub-in: queries ints 2^-133, fp32 subnormals as well)."""
	import test_gpu_ivf_exact as iv
	dev = torch.device("cuda")
	eq, ex = (-79, -70) if name == "all-sub" else (-133, 110)
	g = np.random.default_rng(len(name))
	sizes = np.asarray(IVF_SIZES, dtype=np.int64)
	nq, nprobe, k, dp, vr = 70, 3, 64, 48, 4
	nlist = len(sizes)
	pv = ((np.arange(nq)[:, None] * 3 + np.arange(nprobe)[None, :] * 2) % nlist).astype(np.int32)     # distinct valid lists per row
	n = int(sizes.sum())
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X, Q = g.integers(-vr, vr + 1, (n, dp)).astype(np.int64), g.integers(-vr, vr + 1, (nq, dp)).astype(np.int64)
	Xf, Qf, Xb = _ivf_tensor(X, ex, F32, dev, 8), _ivf_tensor(Q, eq, F32, dev, 0), _ivf_tensor(X, ex, BF16, dev, 8)
	off_d, ids_d, pv_d = torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(pv).to(dev)
	lmax = -(-int(sizes.max()) // 8) * 8
	want = iv._reference(X, Q, off, ids, pv, k, ("slotted", "id"), lmax)
	got = iv._poisoned(ops, lambda: ops.ivf_scan_grouped(Xf, off_d, ids_d, sizes, Qf, pv_d, k))
	_ivf_equal(got, want["slotted"], eq + ex, f"ivf_scan_grouped fp32 {name}")
	got = iv._poisoned(ops, lambda: ops.ivf_scan_grouped(Xf, off_d, ids_d, sizes, Qf, pv_d, k, lists_bf16=Xb))
	_ivf_equal(got, want["slotted"], eq + ex, f"ivf_scan_grouped bf16 lists {name}")
	got = ops.ivf_scan(Xf, off_d, ids_d, Qf, pv_d, k)
	torch.cuda.synchronize()
	_ivf_equal(got, want["id"], eq + ex, f"ivf_scan {name}")


# ------------------------------------------------------------------ 10. the fp64 gather of lstsq_rows
@pytest.mark.parametrize("Q", [1, 5])
def test_lstsq_rows_gathers_subnormal_fp32_into_normal_fp64(ops, Q):
	"""The item-side Hadamard case of tests/test_gpu_lstsq_rows.py at g = 64 with Rt = +-2^-127 -- an fp32 subnormal that widens to a normal
	fp64 -- and C = ints 2^-30: G = 64 2^-254 I, and W = (S / 64) 2^97 in closed form, every fp64 intermediate exact.  A gather that read the
	subnormal as zero would give G = 0 and fail every pivot (status 1, W = NaN)."""
	import test_gpu_lstsq_rows as lr
	g = 64
	pos = (0, g // 2, g - 1)
	cols = list(np.random.default_rng(g).permutation(g)[:g - 3])
	Rt1, ids, C1, S = lr.hadamard_case(g, cols, Q, seed=10 * g + Q, hole_pos=pos)
	host = Rt1.cpu().numpy()
	rows = {i: (host[i].astype(np.float64) * 2.0 ** -127).astype(np.float32) for i in range(host.shape[0]) if np.isfinite(host[i]).all()}
	assert len(rows) == g - 3 and all(sn.is_subnormal(v).all() and (np.abs(v) == np.float32(2.0 ** -127)).all() for v in rows.values())
	Rt = lr.nan_backed_rt(rows, host.shape[0], g)
	assert np.array_equal(sn.bits32(Rt.cpu().numpy()[sorted(rows)]), sn.bits32(np.stack([rows[i] for i in sorted(rows)])))   # the upload kept the subnormals
	C = torch.from_numpy((C1.cpu().numpy().astype(np.float64) * 2.0 ** -30).astype(np.float32)).cuda()
	W, status = lr.run_poisoned(ops, Rt, ids, C, 0.0, False)
	want = (lr.exact_f32(S, g).astype(np.float64) * 2.0 ** 97).astype(np.float32)
	assert np.isfinite(want).all() and (want != 0).mean() > 0.9
	assert np.array_equal(status, np.zeros(Q, dtype=np.int32)), f"status {status.tolist()}: a pivot failed (G = 0 where Rt is read as zero)"
	assert np.array_equal(sn.bits32(W), sn.bits32(want))
