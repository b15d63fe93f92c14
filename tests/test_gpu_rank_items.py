"""Ranks of given items on the device, held BIT FOR BIT to tests/rank_numpy.py: no tolerance anywhere.

G1  anncur_rank_in_rows on fp32 and bf16 rows of integers in [-8, 8] (tie-heavy), pitch > I and odd (rows start at every alignment, so the
    scalar head, the 16-byte body and the tail all run): (Q, I) = (1, 1), (3, 31), (5, 33), (4, 4101), (9, 70 001); t = 1, 7, 64, 1024 with ids
    repeated where I is smaller; holes and duplicates; a row with a NaN block, one with +-inf and signed zeros, one whose targets are all
    the worst items (every element passes the prefilter); 0xff guards behind rank and score; and the inverse of rowwise_topk on Gaussian rows.
G2  anncur_score_rank on integer operands in [-4, 4] (every product and sum exact, so any summation order gives the fp64 result): Kp = 64 ..
    512 with K = Kp and Kp - 3, Q = 1, 70, 257 (129 at Kp = 512), I = 5, 32, 37, 4101, t = 1, 100, 1024 with holes and duplicates; all scores
    negative with I % 32 != 0 (a padded row scores 0 and would be ahead of every target); the score output; a workspace filled with 0xff
    and guarded; the same ranks from rank_dense.
G3  self-consistency on floats: 256 Gaussian bf16 items followed by the same 256 again, every item a target: each row of ranks is a
    permutation and the copy stands right behind its original, with bit-equal scores.  A target score from any other arithmetic than the
    counting pass' own fails this on the first rows.
G4  against the top-k: rank < k <=> id in score_topk_fused(...).indices on rows whose k-th and (k+1)-th scores differ (integer data,
    item-order operand, no leading sample), and the same for rank_dense against score_topk_dense on Gaussian fp32 data over all rows.
G5  the index classes: CURApprox / CURRowIndex with compute_dtype fp32, bf16, bf16x3 and FlatIPIndex fp32 / bf16: the route taken, and the ranks
    against rank_ref of that route's own scores.
Needs an MI355X."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_numpy as rn  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64   # elements of 0xff behind every output


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


def _ptr(t):
	return ctypes.c_void_p(t.data_ptr())


def _guarded(n, dtype):
	buf = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")     # every byte 0xff
	return buf.view(dtype) if dtype != torch.int32 else buf


def _guards_intact(*bufs_n):
	for buf, n in bufs_n:
		assert (buf.view(torch.int32)[n:] == -1).all(), "bytes behind an output were written"


def _raw_rank_in_rows(S_dev, I, ids_dev):
	"""The library call on guarded outputs: S_dev [Q x pitch] (a padded buffer, the row is its first I elements) -> (rank, score) NumPy."""
	from anncur_amd import _lib
	Q, t = ids_dev.shape
	rank, score = _guarded(Q * t, torch.int32), _guarded(Q * t, torch.float32)
	dt = _lib.F32 if S_dev.dtype == torch.float32 else _lib.BF16
	_lib.check(_lib.load().anncur_rank_in_rows(_ptr(S_dev), dt, Q, I, S_dev.stride(0), _ptr(ids_dev), t, _ptr(rank), _ptr(score),
												ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "rank_in_rows")
	torch.cuda.synchronize()
	_guards_intact((rank, Q * t), (score, Q * t))
	return rank[:Q * t].reshape(Q, t).cpu().numpy(), score[:Q * t].reshape(Q, t).cpu().numpy()


def _want_scores(S, ids):
	w = np.take_along_axis(S, np.maximum(ids, 0).astype(np.int64), axis=1).astype(np.float32)
	w[ids < 0] = np.nan
	return w


def _same_bits(a, b):
	return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32) & np.where(np.isnan(a), 0, 0xffffffff).astype(np.uint32),
						  np.asarray(b, dtype=np.float32).view(np.uint32) & np.where(np.isnan(b), 0, 0xffffffff).astype(np.uint32)) \
		and np.array_equal(np.isnan(a), np.isnan(b))


# ------------------------------------------------------------------ G1
def _tie_heavy_rows(Q, I, seed):
	rng = np.random.default_rng(seed)
	S = rng.integers(-8, 9, (Q, I)).astype(np.float32)
	if I >= 31:
		S[0, 5:20] = np.nan                                                  # a NaN block (with the default and the sign-bit payload)
		S[0, 7:9] = np.array([0xffc00000, 0x7fffffff], dtype=np.uint32).view(np.float32)
		r = 1 % Q
		S[r, 21], S[r, 22], S[r, 23], S[r, 24], S[r, 25], S[r, 26] = np.inf, -np.inf, -0.0, 0.0, -0.0, np.inf
		S[r, I - 1] = -np.inf
	return S


def _targets(S, t, seed, worst_row=None):
	Q, I = S.shape
	rng = np.random.default_rng(seed)
	ids = rng.integers(0, I, (Q, t)).astype(np.int32)                           # t > I repeats ids; duplicates anyway
	if t >= 7:
		ids[:, 3] = -1                                                       # a hole in every row
		ids[:, 5] = ids[:, 4]                                                # an adjacent duplicate
		if I >= 31:
			ids[0, :3] = (5, 7, 8)                                           # NaN targets
			ids[1 % Q, :3] = (21, 22, 23)
			ids[1 % Q, 6] = 24
	if worst_row is not None:                                                # the t worst items of the row: every element is ahead of one of them
		order = np.argsort(-np.nan_to_num(S[worst_row], nan=-np.inf), kind="stable")
		ids[worst_row] = np.resize(order[::-1][:min(t, I)], t)
	return ids


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Q, I", [(1, 1), (3, 31), (5, 33), (4, 4101), (9, 70001)])
def test_g1_rank_in_rows_tie_heavy(gpu, dtype, Q, I):
	from anncur_amd import ops
	S = _tie_heavy_rows(Q, I, seed=I)
	pitch = I + 3                                                            # odd: successive rows start at different offsets inside 16 bytes
	S_dev = torch.full((Q, pitch), 99.0, dtype=dtype, device="cuda")           # the padding would be ahead of everything if it were counted
	S_dev[:, :I] = torch.from_numpy(S).to(dtype).cuda()                      # integers in [-8, 8], +-inf, NaN: exact in bf16
	for t in (1, 7, 64, 1024):
		worst = Q - 1 if Q >= 3 and t >= 7 else None
		ids = _targets(S, t, seed=t, worst_row=worst)
		want = rn.rank_ref(S, ids)
		rank, score = _raw_rank_in_rows(S_dev, I, torch.from_numpy(ids).cuda())
		assert np.array_equal(rank, want), (t, np.argwhere(rank != want)[:5])
		assert _same_bits(score, _want_scores(S, ids)), t
		if t >= 7 and I >= 31:                                                 # (the reference itself: holes, NaN targets, +inf first, duplicates)
			rows = [q for q in range(Q) if q != worst]
			assert (want[rows, 3] == -1).all() and (want[0, :3] == -1).all() and want[1 % Q, 0] == 0 and (want[rows, 4] == want[rows, 5]).all()
	# the binding: a strided view of the padded buffer, ids on the host or on the device, with and without scores
	ids = _targets(S, 7, seed=7)
	want = rn.rank_ref(S, ids)
	assert np.array_equal(ops.rank_in_rows(S_dev[:, :I], ids).cpu().numpy(), want)
	r, s = ops.rank_in_rows(S_dev[:, :I], torch.from_numpy(ids).cuda(), return_scores=True)
	assert r.dtype == torch.int32 and s.dtype == torch.float32 and np.array_equal(r.cpu().numpy(), want) and _same_bits(s.cpu().numpy(), _want_scores(S, ids))


def test_g1_every_element_is_a_survivor(gpu):
	"""Targets = the worst items of each row, so the whole row goes through the binary search; with t = 1024 distinct targets in a row of
	4101 the bins see up to ~3000 counts each side."""
	rng = np.random.default_rng(3)
	S = rng.integers(-8, 9, (3, 4101)).astype(np.float32)
	order = np.argsort(-S, axis=1, kind="stable")
	ids = np.ascontiguousarray(order[:, ::-1][:, :1024]).astype(np.int32)
	S_dev = torch.from_numpy(S).cuda()
	rank, _ = _raw_rank_in_rows(S_dev, 4101, torch.from_numpy(ids).cuda())
	assert np.array_equal(rank, rn.rank_ref(S, ids)) and np.array_equal(rank, np.tile(np.arange(4100, 4100 - 1024, -1, dtype=np.int32), (3, 1)))


@pytest.mark.parametrize("k", [10, 128, 300])
def test_g1_inverse_of_rowwise_topk(gpu, k):
	from anncur_amd import ops
	g = torch.Generator().manual_seed(k)
	A = torch.randn(6, 5003, generator=g).cuda()
	top = ops.rowwise_topk(A, k)
	rank, score = ops.rank_in_rows(A, top.indices, return_scores=True)
	assert torch.equal(rank, torch.arange(k, dtype=torch.int32, device="cuda").expand(6, k))
	assert torch.equal(score, top.values)


# ------------------------------------------------------------------ G2
def _int_case(Q, I, K, seed, x_lo=-4, x_hi=4, e_lo=-4, e_hi=4):
	rng = np.random.default_rng(seed)
	X = rng.integers(x_lo, x_hi + 1, (Q, K)).astype(np.float32)
	E = rng.integers(e_lo, e_hi + 1, (I, K)).astype(np.float32)
	return X, E, X.astype(np.float64) @ E.astype(np.float64).T              # |S| <= 16 K <= 8192: exact in fp32 in any order


def _ids_with_holes(Q, I, t, seed):
	rng = np.random.default_rng(seed)
	ids = rng.integers(0, I, (Q, t)).astype(np.int32)
	if t >= 100:
		ids[:, 1::17] = -1
		ids[:, 2] = ids[:, 0]
	return ids


def _poisoned_workspace(nbytes):
	buf = torch.full((nbytes + 256 + 4 * GUARD,), 0xff, dtype=torch.uint8, device="cuda")
	off = (-buf.data_ptr()) % 256
	return buf[off:off + nbytes], buf[off + nbytes:]


def _score_rank_checked(ops, X, E, S, ids, Kp):
	"""score_rank on a 0xff-filled, guarded workspace: ranks against rank_ref of the fp64 scores, the score output exact; then rank_dense."""
	from anncur_amd import _lib
	Q, I = S.shape
	Xp, Etp = ops.pack_bf16(torch.from_numpy(X).cuda(), Kp), ops.pack_bf16(torch.from_numpy(E).cuda(), Kp, row_multiple=32)
	assert Etp.shape[0] == -(-I // 32) * 32 and not Etp[I:].any()
	ws, guard = _poisoned_workspace(_lib.load().anncur_score_rank_workspace_bytes(Q, I, Kp, ids.shape[1]))
	rank, score = ops.score_rank(Xp, Etp, I, torch.from_numpy(ids).cuda(), return_scores=True, workspace=ws)
	torch.cuda.synchronize()
	assert (guard == 0xff).all(), "bytes behind the workspace were written"
	want = rn.rank_ref(S, ids)
	got = rank.cpu().numpy()
	assert np.array_equal(got, want), (Q, I, Kp, ids.shape[1], np.argwhere(got != want)[:5])
	assert _same_bits(score.cpu().numpy(), _want_scores(S, ids)), (Q, I, Kp)
	dense = ops.rank_dense(torch.from_numpy(X).cuda(), torch.from_numpy(E).cuda(), ids)
	assert np.array_equal(dense.cpu().numpy(), want), (Q, I, Kp, "rank_dense")


@pytest.mark.parametrize("Kp, K", [(kp, k) for kp in (64, 128, 256, 512) for k in (kp, kp - 3)])
def test_g2_score_rank_integer_operands(gpu, Kp, K):
	from anncur_amd import ops
	seed = 0
	for Q in (1, 70, 129 if Kp == 512 else 257):                              # one lane, a ragged block, one row past a block
		for I in (5, 32, 37, 4101):                                          # Q = 1, I = 4101: the item range splits over workgroups
			X, E, S = _int_case(Q, I, K, seed=1000 * Kp + K + Q + I)
			for t in (1, 100, 1024):
				seed += 1
				_score_rank_checked(ops, X, E, S, _ids_with_holes(Q, I, t, seed), Kp)


@pytest.mark.parametrize("Kp, Q, I", [(64, 70, 37), (128, 5, 4101), (256, 33, 5), (512, 129, 95)])
def test_g2_all_scores_negative_padded_rows_are_not_counted(gpu, Kp, Q, I):
	"""X > 0, E < 0: every score is negative and I % 32 != 0, so the zero rows that pad Et to a tile score 0 -- ahead of every target if
	they were counted.  The best item of every query must still get rank 0."""
	from anncur_amd import ops
	assert I % 32 != 0
	X, E, S = _int_case(Q, I, Kp - 3, seed=Kp + I, x_lo=1, x_hi=4, e_lo=-4, e_hi=-1)
	assert (S < 0).all()
	ids = np.concatenate([np.argmax(S, axis=1)[:, None], _ids_with_holes(Q, I, 100, Kp)], axis=1).astype(np.int32)
	assert (rn.rank_ref(S, ids)[:, 0] == 0).all()
	_score_rank_checked(ops, X, E, S, ids, Kp)


def test_g2_default_workspace_and_strided_queries(gpu):
	"""The shared grow-only workspace (whatever an earlier call left in it), a query operand whose rows are not packed, int32 ids on the host."""
	from anncur_amd import ops
	X, E, S = _int_case(70, 1000, 64, seed=5)
	Etp = ops.pack_bf16(torch.from_numpy(E).cuda(), 64, row_multiple=32)
	wide = torch.full((70, 64 + 24), 7.0, dtype=torch.bfloat16, device="cuda")
	wide[:, :64] = ops.pack_bf16(torch.from_numpy(X).cuda(), 64)
	ids = _ids_with_holes(70, 1000, 100, 9)
	want = rn.rank_ref(S, ids)
	for _ in range(2):                                                        # the second call meets the first call's leftovers
		assert np.array_equal(ops.score_rank(wide[:, :64], Etp, 1000, ids).cpu().numpy(), want)


# ------------------------------------------------------------------ G3
def test_g3_self_consistency_on_floats(gpu):
	from anncur_amd import ops
	n, K, Q = 256, 256, 70
	g = torch.Generator().manual_seed(11)
	E = torch.randn(n, K, generator=g).bfloat16()
	X = torch.randn(Q, K, generator=g).bfloat16()
	Etp = ops.pack_bf16(torch.cat([E, E]).cuda(), K, row_multiple=32)
	Xp = ops.pack_bf16(X.cuda(), K)
	ids = torch.arange(2 * n, dtype=torch.int32).expand(Q, 2 * n).contiguous()
	rank, score = ops.score_rank(Xp, Etp, 2 * n, ids, return_scores=True)
	rank, score = rank.cpu().numpy(), score.cpu().numpy()
	assert np.array_equal(np.sort(rank, axis=1), np.tile(np.arange(2 * n, dtype=np.int32), (Q, 1)))       # every row a permutation of 0..511
	assert np.array_equal(rank[:, n:], rank[:, :n] + 1)                                                     # the copy stands right behind its original
	assert np.array_equal(score[:, n:].view(np.uint32), score[:, :n].view(np.uint32))
	assert np.array_equal(rank, rn.rank_ref(score, ids.numpy()))                                            # and the ranks are those of the reported scores
	assert len(np.unique(score[0, :n])) > n // 2                                                            # (floats, not a tie-heavy toy)


# ------------------------------------------------------------------ G4
def test_g4_rank_below_k_iff_in_the_fused_topk(gpu):
	from anncur_amd import ops
	Q, I, Kp, k = 300, 20000, 256, 100
	rng = np.random.default_rng(4)
	X = rng.integers(0, 5, (Q, Kp)).astype(np.float32)
	E = rng.integers(-4, 5, (I, Kp)).astype(np.float32)
	S = X @ E.T                                                              # |S| <= 4096: exact
	srt = -np.sort(-S, axis=1)
	clear = np.flatnonzero(srt[:, k - 1] != srt[:, k])                        # rows whose k-th and (k+1)-th best scores differ: the top-k is one SET
	assert clear.size >= 20, clear.size
	Xp, Etp = ops.pack_bf16(torch.from_numpy(X).cuda(), Kp), ops.pack_bf16(torch.from_numpy(E).cuda(), Kp, row_multiple=32)
	assert ops.fused_supported(Q, I, Kp, k)
	top = ops.score_topk_fused(Xp, Etp, I, k).indices.cpu().numpy()
	order = np.argsort(-S, axis=1, kind="stable")
	ids = np.concatenate([order[:, :150], rng.integers(0, I, (Q, 50))], axis=1).astype(np.int32)          # around the boundary, and anywhere
	rank = ops.score_rank(Xp, Etp, I, ids).cpu().numpy()
	assert np.array_equal(rank, rn.rank_ref(S, ids))
	for q in clear:
		assert np.array_equal(rank[q] < k, np.isin(ids[q], top[q])), q


def test_g4_rank_dense_against_score_topk_dense(gpu):
	"""Gaussian fp32 data, all rows: both sides score with the same fmaf chain (ops.gemm) and both break ties by id."""
	from anncur_amd import ops
	Q, I, K, k = 64, 3001, 48, 50
	g = torch.Generator().manual_seed(6)
	X, E = torch.randn(Q, K, generator=g).cuda(), torch.randn(I, K, generator=g).cuda()
	top = ops.score_topk_dense(X, E, k)
	rank, score = ops.rank_dense(X, E, top.indices, return_scores=True)
	assert torch.equal(rank, torch.arange(k, dtype=torch.int32, device="cuda").expand(Q, k)) and torch.equal(score, top.values)
	ids = torch.randint(0, I, (Q, 200), generator=g, dtype=torch.int32)
	rank = ops.rank_dense(X, E, ids, max_bytes=4 * I * 10).cpu().numpy()      # seven row chunks
	topi = top.indices.cpu().numpy()
	for q in range(Q):
		assert np.array_equal(rank[q] < k, np.isin(ids[q].numpy(), topi[q])), q
	assert np.array_equal(rank, rn.rank_ref(ops.gemm(X, E.t()).cpu().numpy(), ids.numpy()))


# ------------------------------------------------------------------ G5
def _cur_data():
	"""Integer scores of the size of tests/golden/lr_200x1000.npz: 200 training queries, 1000 items, 60 test queries, rank 8 plus integer noise."""
	rng = np.random.default_rng(12)
	A = (rng.integers(-3, 4, (260, 8)) @ rng.integers(-3, 4, (8, 1000)) + rng.integers(-1, 2, (260, 1000))).astype(np.float32)
	anc = sorted(int(i) for i in rng.choice(1000, 40, replace=False))
	ids = rng.integers(-1, 1000, (60, 50)).astype(np.int32)
	ids[:, 7] = ids[:, 6]
	return torch.from_numpy(A[:200]).cuda(), torch.from_numpy(A[200:]).cuda(), anc, ids


def _route_scores(ops, op, X, route):
	"""The scores the route itself ranks, for EVERY item: the dense route's are ops.gemm on the fp32 operand; the fused route's are what
	score_rank reports when every item is a target (m = 1000 <= RANK_MAX_T)."""
	if route == "dense":
		return ops.gemm(X if X.dtype == torch.float32 else ops.convert(X, torch.float32), op._Et.t()).cpu().numpy()
	every = torch.arange(op.m, dtype=torch.int32).expand(X.shape[0], op.m).contiguous()
	return ops.score_rank(ops.pack_bf16(X, op._Etp.shape[1]), op._Etp, op.m, every, return_scores=True)[1].cpu().numpy()


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16", "bf16x3"])
def test_g5_cur_classes(gpu, compute_dtype):
	from anncur_amd import ops
	from anncur_amd.cur import CURApprox, CURRowIndex
	A_train, A_test, anc, ids = _cur_data()
	route = "bf16" if compute_dtype == "bf16" else "dense"
	X = ops.gather_cols(A_test, anc)
	index = CURRowIndex(A_train, np.asarray(anc), compute_dtype=compute_dtype, pinv_backend="numpy")
	assert index.rank_route(50) == route and index.rank_route(1025) == "dense"
	S = _route_scores(ops, index, X, route)
	want = rn.rank_ref(S, ids)
	got = index.rank_of(X, ids)
	assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
	r, s = index.rank_of(X, torch.from_numpy(ids).long().cuda(), return_scores=True)                          # int64 ids on the device
	assert np.array_equal(r.cpu().numpy(), want) and _same_bits(s.cpu().numpy(), _want_scores(S, ids))
	# the ranks of the index' own top-k are 0..k-1 where the top-k ranks the same scores and breaks ties by id: the dense fp32 route
	if compute_dtype == "fp32":
		top = index.topk(X, 20)
		assert torch.equal(index.rank_of(X, top.indices), torch.arange(20, dtype=torch.int32, device="cuda").expand(60, 20))
	cur = CURApprox(rows=A_train, cols=ops.gather_cols(A_train, anc), row_idxs=np.arange(200), col_idxs=anc, approx_preference="rows", compute_dtype=compute_dtype,
					pinv_backend="numpy")
	assert cur.rank_route(50) == route
	assert np.array_equal(cur.rank_in_row(X, ids).cpu().numpy(), rn.rank_ref(_route_scores(ops, cur, X, route), ids))
	got = cur.rank_in_row(X.cpu(), ids)                                                                    # CPU in -> CPU out, like topk_in_row
	assert not got.is_cuda and np.array_equal(got.numpy(), rn.rank_ref(_route_scores(ops, cur, X, route), ids))
	cols = CURApprox(rows=A_train, cols=ops.gather_cols(A_train, anc), row_idxs=np.arange(200), col_idxs=anc, approx_preference="cols", pinv_backend="numpy")
	with pytest.raises(NotImplementedError):
		cols.rank_in_row(X, ids)


@pytest.mark.parametrize("dtype, d", [("fp32", 24), ("bf16", 24), ("bf16", 130), ("bf16x3", 24)])
def test_g5_flat_index(gpu, dtype, d):
	from anncur_amd.nearest_nbr import FlatIPIndex
	rng = np.random.default_rng(d)
	E = rng.integers(-8, 9, (1500, d)).astype(np.float32)                      # integers: exact in bf16 and in any summation order
	q = rng.integers(-8, 9, (33, d)).astype(np.float32)
	ids = rng.integers(-1, 1500, (33, 64)).astype(np.int32)
	index = FlatIPIndex(d, dtype=dtype)
	index.add(E[:700])
	index.add(E[700:])
	assert index.rank_route(64) == ("bf16" if dtype == "bf16" else "dense")
	got = index.rank(q, ids)
	assert isinstance(got, np.ndarray) and got.dtype == np.int32
	assert np.array_equal(got, rn.rank_ref(q.astype(np.float64) @ E.astype(np.float64).T, ids))
	if dtype == "bf16":
		assert tuple(index._rank_op()._Etp.shape) == (1504, 64 if d == 24 else 256) and index._Xp is None   # an item-order copy of its own, built lazily
	D, top = index.search(q, 10)
	if dtype == "fp32":                                                        # (the dense search ranks the same scores and breaks ties by id)
		assert np.array_equal(index.rank(q, top.astype(np.int32)), np.tile(np.arange(10, dtype=np.int32), (33, 1)))
	index.add(E[:5])
	assert index._rank_operand is None and index.rank(q, ids[:, :3]).shape == (33, 3)                        # add() drops the copy
