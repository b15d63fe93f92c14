"""The sparse inner-product route on the device (csrc/sparse.hip) against tests/sparse_numpy.py and tests/topk_numpy.py, BIT FOR BIT:
every comparison goes through integer views.  The shapes are the smallest that reach the kernel's four edges: the 2048-item window and
the span of windows a wave owns, the 64-term pass, the 64-item group, and the cursor a wave carries from one window to the next (which
needs Q x windows > 2048 waves: Q = 700 on 4 windows, Q = 65 on 41)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_numpy as sn  # noqa: E402
from topk_numpy import topk_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
	from anncur_amd import ops as _ops
	assert torch.cuda.is_available()
	return _ops


def _bits(a):
	a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
	return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
	g, w = _bits(got), _bits(want)
	assert g.shape == w.shape, (what, g.shape, w.shape)
	bad = np.argwhere(g != w)
	assert bad.size == 0, f"{what}: {len(bad)} of {g.size} differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]:#010x}, want {w[tuple(bad[0])]:#010x}"


def _postings(ops, items):
	return ops.sparse_postings(*items.triple, items.shape[0], items.shape[1])


def _check_rows(ops, queries, items, ref, what):
	S, GM = ops.sparse_score_rows(queries, _postings(ops, items))
	torch.cuda.synchronize()
	_same_bits(S, ref, what + ": S")
	_same_bits(GM, sn.group_maxima(ref), what + ": GM")
	return S


def _check_topk(ops, got, ref, k, what):
	val, idx = got.values.cpu().numpy(), got.indices.cpu().numpy()
	assert val.shape == idx.shape == (ref.shape[0], k) and idx.dtype == np.int32
	for q in range(ref.shape[0]):
		wv, wi = topk_ref(ref[q], k)
		assert np.array_equal(idx[q], wi), f"{what}: ids of query {q} differ at {np.flatnonzero(idx[q] != wi)[:5].tolist()}"
		_same_bits(val[q], wv, f"{what}: values of query {q}")


# ================================================================== 1. integer data at every edge of the window, the group and the term pass
@pytest.mark.parametrize("V", [1, 7, 300])
@pytest.mark.parametrize("I", [1, 63, 64, 65, 2047, 2048, 2049, 4101, 3 * 2048 + 5])
def test_integer_data(ops, I, V):
	for Q in (1, 3, 65):
		rng = np.random.default_rng([I, V, Q])
		items = sn.integer_csr(rng, I, V, 0, 12)
		queries = sn.integer_csr(rng, Q, V, 0, 40)
		ref = sn.scores_ref(queries, items)
		dense = sn.densify(queries).astype(np.int64) @ sn.densify(items).astype(np.int64).T
		assert np.array_equal(ref.astype(np.int64), dense) and not (_bits(ref) == 0x80000000).any()
		_check_rows(ops, queries, items, ref, f"I={I} V={V} Q={Q}")
		post = _postings(ops, items)
		for k in sorted({1, min(10, I), min(100, I), min(I, 2048)}):
			_check_topk(ops, ops.sparse_score_topk(queries, post, k), ref, k, f"I={I} V={V} Q={Q} k={k}")


@pytest.mark.parametrize("Q,I", [(700, 3 * 2048 + 5), (65, 40 * 2048 + 5)])
def test_cursors_carried_between_the_windows_of_a_span(ops, Q, I):
	"""More than 2048 (query, window) pairs: a wave owns two windows and takes the second one's start from where the first one's walk ended."""
	assert ops.sparse_plan(Q, I)["windows_per_wave"] == 2 and ops.sparse_plan(Q, I)["windows"] % 2 == (0 if Q == 700 else 1)
	rng = np.random.default_rng(Q)
	items = sn.integer_csr(rng, I, 7, 0, 7)
	queries = sn.integer_csr(rng, Q, 7, 1, 7)
	ref = sn.scores_ref(queries, items)
	assert np.array_equal(ref.astype(np.int64), sn.densify(queries).astype(np.int64) @ sn.densify(items).astype(np.int64).T)
	_check_rows(ops, queries, items, ref, f"Q={Q} I={I}")
	_check_topk(ops, ops.sparse_score_topk(queries, _postings(ops, items), 10), ref, 10, f"Q={Q} I={I} k=10")


# ================================================================== 2. the summation order
@pytest.fixture(scope="module")
def real_case():
	rng = np.random.default_rng(20)
	queries, items = sn.real_csr(rng, 5, 300, 20, 89), sn.real_csr(rng, 4101, 300, 1, 39)
	return queries, items, sn.scores_ref(queries, items)


def test_scores_are_the_ascending_term_chain(ops, real_case):
	queries, items, ref = real_case
	down = sn.scores_ref(queries, items, descending=True)
	assert (_bits(ref) != _bits(down)).any()          # the data can tell the orders apart (tests/test_cpu_sparse_host.py counts them)
	S = _check_rows(ops, queries, items, ref, "real-valued data")
	assert (_bits(S) != _bits(down)).any()
	post = _postings(ops, items)
	for k in (1, 100, 2048):
		_check_topk(ops, ops.sparse_score_topk(queries, post, k), ref, k, f"real-valued data, k={k}")


# ================================================================== 3. query lengths around the 64-term pass
def test_query_lengths_around_the_term_pass(ops):
	V, I = 1500, 4101
	rng = np.random.default_rng(3)
	items = sn.integer_csr(rng, I, V, 1, 30)
	lengths = [0, 1, 63, 64, 65, 129, ops.SPARSE_MAX_QNNZ]
	rows = []
	for n in lengths:
		rows.append((np.sort(rng.choice(V, size=n, replace=False)), rng.integers(-8, 9, n).astype(np.float32)))
	queries = sn.csr_from_rows(rows, V)
	ref = sn.scores_ref(queries, items)
	assert np.array_equal(ref.astype(np.int64), sn.densify(queries).astype(np.int64) @ sn.densify(items).astype(np.int64).T)
	S = _check_rows(ops, queries, items, ref, "query lengths")
	assert not _bits(S[0]).any()                       # the empty query: +0.0 everywhere, bit pattern 0
	post = _postings(ops, items)
	for k in (1, 10, 100):
		got = ops.sparse_score_topk(queries, post, k)
		_check_topk(ops, got, ref, k, f"query lengths, k={k}")
		assert got.indices[0].cpu().tolist() == list(range(k)) and not _bits(got.values[0]).any()


# ================================================================== 4. postings at the edges
def test_postings_at_the_edges_of_windows_and_lists(ops):
	I, V = 3 * 2048 + 5, 10
	empty_item = 100
	rng = np.random.default_rng(4)
	rows = []
	for i in range(I):
		t, v = [0], [float(rng.integers(1, 9))]                    # term 0: in every item (but one), across every window
		for term, item in ((1, 0), (2, 2047), (3, 2048), (4, I - 1)):   # terms 1..4: a single posting each
			if i == item:
				t.append(term); v.append(float(term))
		# term 5: no posting at all.  terms 6 and 7: equal and opposite on every 5th item.  term 8: stored zeros on every 7th item
		if i % 5 == 0:
			t += [6, 7]; v += [3.0, -3.0]
		if i % 7 == 0:
			t.append(8); v.append(0.0)
		rows.append(([], []) if i == empty_item else (t, v))
	items = sn.csr_from_rows(rows, V)
	queries = sn.csr_from_rows([
		(list(range(10)), [1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
		([5], [2.0]),                                  # only the empty list: every score +0.0
		([1, 2, 3, 4], [1, -1, 1, -1]),
		([6, 7], [2.0, 2.0]),                          # 6 + (-6): +0.0, never -0.0
		([8], [-1.0]),                                 # -1 x 0 = -0.0, and +0.0 + -0.0 = +0.0
		([0, 5, 9], [-1.0, 1.0, 1.0]),                 # all negative but the empty item: zero ranks first
		([6, 7, 8], [1.0, 1.0, -4.0]),
	], V)
	ref = sn.scores_ref(queries, items)
	assert np.array_equal(ref.astype(np.int64), sn.densify(queries).astype(np.int64) @ sn.densify(items).astype(np.int64).T)
	assert not (_bits(ref) == 0x80000000).any() and not _bits(ref[[1, 3, 4, 6]]).any()
	assert ref[2, 0] == 1 and ref[2, 2047] == -2 and ref[2, 2048] == 3 and ref[2, I - 1] == -4 and np.count_nonzero(ref[2]) == 4
	S = _check_rows(ops, queries, items, ref, "edges")
	assert not (_bits(S) == 0x80000000).any()
	post = _postings(ops, items)
	for k in (1, 5, 100, 2048):
		got = ops.sparse_score_topk(queries, post, k)
		_check_topk(ops, got, ref, k, f"edges, k={k}")
		assert got.indices[5, 0].item() == empty_item and got.indices[1].cpu().tolist() == list(range(k))
	assert ops.sparse_score_topk(queries, post, 5).indices[2].cpu().tolist() == [2048, 0, 1, 2, 3]


# ================================================================== 5. ties and sign
def test_zeros_rank_by_id_above_every_negative_score(ops):
	I = 3 * 2048 + 5
	pos = {5000: 2.0, 17: 7.0, 2048: 7.0}
	rows = []
	for i in range(I):
		if i in pos:
			rows.append(([0], [pos[i]]))
		elif i % 3 == 1:
			rows.append(([0], [-float(1 + i % 5)]))
		else:
			rows.append(([1], [1.0]))                  # shares nothing with the query: +0.0
	items = sn.csr_from_rows(rows, 2)
	queries = sn.csr_from_rows([([0], [1.0])], 2)
	ref = sn.scores_ref(queries, items)
	zeros = np.flatnonzero(ref[0] == 0)
	assert zeros.size > 4000 and (ref[0] < 0).sum() > 2000 and (ref[0] > 0).sum() == 3
	_check_rows(ops, queries, items, ref, "ties")
	post = _postings(ops, items)
	for k in (2, 3, 4, 100, 2048):
		got = ops.sparse_score_topk(queries, post, k)
		_check_topk(ops, got, ref, k, f"ties, k={k}")
		ids = got.indices[0].cpu().numpy()
		assert ids[:min(k, 3)].tolist() == [17, 2048, 5000][:min(k, 3)] and np.array_equal(ids[3:], zeros[:max(k - 3, 0)])
	# more than all non-negative items: the negatives follow the zeros, the least negative first, ties by id
	items2 = sn.csr_from_rows(rows[:300], 2)
	ref2 = sn.scores_ref(queries, items2)
	got = ops.sparse_score_topk(queries, _postings(ops, items2), 300)
	_check_topk(ops, got, ref2, 300, "ties, k = I")
	v = got.values[0].cpu().numpy()
	assert (np.diff(v) <= 0).all() and v[-1] == -5 and (v == 0).sum() == (ref2[0] == 0).sum()


# ================================================================== 6. chunking and shape independence
def test_results_do_not_depend_on_chunks_or_positions(ops, real_case):
	_, items, _ = real_case
	rng = np.random.default_rng(6)
	queries = sn.real_csr(rng, 65, 300, 0, 89)
	ref = sn.scores_ref(queries, items)
	post = _postings(ops, items)
	k = 100
	whole = ops.sparse_score_topk(queries, post, k)
	_check_topk(ops, whole, ref, k, "65 queries in one call")
	one = ops.sparse_score_topk(queries, post, k, max_bytes=1)           # one query per chunk
	_same_bits(one.values, whole.values, "chunks of one query: values")
	assert torch.equal(one.indices, whole.indices)
	perm = rng.permutation(65)
	rows = [(queries.indices[queries.indptr[q]:queries.indptr[q + 1]], queries.data[queries.indptr[q]:queries.indptr[q + 1]]) for q in range(65)]
	shuffled = ops.sparse_score_topk(sn.csr_from_rows([rows[p] for p in perm], 300), post, k)
	inv = torch.as_tensor(np.argsort(perm), device="cuda")
	_same_bits(shuffled.values[inv], whole.values, "permuted queries: values")
	assert torch.equal(shuffled.indices[inv], whole.indices)
	S = _check_rows(ops, queries, items, ref, "65 queries")
	for q in (0, 1, 31, 64):
		S1, GM1 = ops.sparse_score_rows(sn.csr_from_rows([rows[q]], 300), post)
		_same_bits(S1[0], S[q], f"query {q} alone: S")
		t1 = ops.sparse_score_topk(sn.csr_from_rows([rows[q]], 300), post, k)
		_same_bits(t1.values[0], whole.values[q], f"query {q} alone: values")
		assert torch.equal(t1.indices[0], whole.indices[q])
	empty = ops.sparse_score_topk(sn.csr_from_rows([], 300), post, k)
	assert tuple(empty.values.shape) == (0, k) and tuple(empty.indices.shape) == (0, k)
	# the same operands as device tensors and as a duck-typed object give the same call
	dev = tuple(torch.as_tensor(a).cuda() for a in queries.triple)
	_same_bits(ops.sparse_score_topk(dev, post, k).values, whole.values, "device triple: values")


# ================================================================== 7. exclude=
def test_exclusion_lists(ops):
	rng = np.random.default_rng(7)
	I, V, Q, k = 2049, 7, 6, 10
	items = sn.integer_csr(rng, I, V, 0, 7)
	queries = sn.integer_csr(rng, Q, V, 1, 7)
	ref = sn.scores_ref(queries, items)
	post = _postings(ops, items)
	best = [topk_ref(ref[q], 8)[1] for q in range(Q)]

	def check(exclude, lists, what, post=post, ref=ref, k=k):
		got = ops.sparse_score_topk(queries, post, k, exclude=exclude)
		masked = ref.copy()
		for q, l in enumerate(lists):
			masked[q, np.asarray(l, dtype=np.int64)] = np.nan       # topk_ref never selects a NaN
		_check_topk(ops, got, masked, k, what)
		return got

	shared = [int(i) for i in best[0][:5]] + [0, I - 1]
	check(shared, [shared] * Q, "one list for all queries")
	per_query = [[int(i) for i in best[q][:q + 1]] for q in range(Q)]
	check(per_query, per_query, "per-query lists")
	padded = np.full((Q, 8), -1, dtype=np.int64)
	for q in range(Q):
		padded[q, :q + 1] = best[q][:q + 1]
	check(padded, per_query, "-1 padded array")
	check(torch.as_tensor(padded), per_query, "-1 padded tensor")
	# k + the longest list = every item: 12 items, query q loses q of them, k = 7 of the 12 - q >= 7 that are left (a call cannot ask for more:
	# k + e_max <= I is a limit of every route, so a row is never left with fewer than k)
	items12 = sn.csr_from_rows([(items.indices[items.indptr[i]:items.indptr[i + 1]], items.data[items.indptr[i]:items.indptr[i + 1]]) for i in range(12)], V)
	ref12, post12 = sn.scores_ref(queries, items12), _postings(ops, items12)
	lists = [list(range(q)) for q in range(Q)]
	got = check(lists, lists, "k + e_max = I", post=post12, ref=ref12, k=7)
	assert (got.indices >= 0).all() and not np.isin(got.indices[5].cpu().numpy(), lists[5]).any()
	with pytest.raises(ValueError, match="candidates per query"):
		ops.sparse_score_topk(queries, post12, 10, exclude=[0, 1, 2])


# ================================================================== 8. poisoned scratch, guards
def test_poisoned_workspace_and_guards(ops, real_case):
	from anncur_amd import _lib
	queries, items, ref = real_case
	Q, I, k = queries.shape[0], items.shape[0], 100
	post = _postings(ops, items)
	ws = ops.sparse_workspace(Q, I, k, torch.device("cuda"))
	ws.fill_(0xff)
	_check_topk(ops, ops.sparse_score_topk(queries, post, k, workspace=ws), ref, k, "0xff-filled workspace")
	with pytest.raises(ValueError, match="workspace too small"):
		ops.sparse_score_topk(queries, post, k, workspace=ws[:ws.numel() - 256])
	# the C ABI on buffers with guards: S at a pitch with 6 guard columns (odd: the scalar-store path) and with 43 (a multiple of 4: 16-byte stores)
	lib = _lib.load()
	q = [torch.as_tensor(a).cuda() for a in queries.triple]
	G = -(-I // 64)
	p = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
	for pad in (6, 43):
		lds, ldg = I + pad, G + 3
		assert (lds % 4 == 0) == (pad == 43)
		S = torch.full((Q + 2, lds), -1, dtype=torch.int32, device="cuda")
		GM = torch.full((Q + 2, ldg), -1, dtype=torch.int32, device="cuda")
		rc = lib.anncur_sparse_score_rows(p(q[0]), p(q[1]), p(q[2]), Q, p(post.term_ptr), p(post.post_item), p(post.post_val), post.n_terms, I,
										  S[1:].data_ptr(), lds, GM[1:].data_ptr(), ldg, torch.cuda.current_stream().cuda_stream)
		torch.cuda.synchronize()
		assert rc == 0, lib.anncur_last_error()
		_same_bits(S[1:Q + 1, :I].contiguous().view(torch.float32), ref, f"S at pitch I + {pad}")
		_same_bits(GM[1:Q + 1, :G].contiguous().view(torch.float32), sn.group_maxima(ref), f"GM at pitch G + 3 (pad {pad})")
		assert (S[0] == -1).all() and (S[Q + 1] == -1).all() and (S[:, I:] == -1).all(), "guard around S"
		assert (GM[0] == -1).all() and (GM[Q + 1] == -1).all() and (GM[:, G:] == -1).all(), "guard around GM"
	# outputs of the top-k call with guards behind them, GM = NULL inside
	nbytes = lib.anncur_sparse_score_topk_workspace_bytes(Q, I, k)
	buf = torch.full((nbytes + 256 + 4096,), 0xff, dtype=torch.uint8, device="cuda")
	off = (-buf.data_ptr()) % 256
	val = torch.full((Q * k + 64,), -1, dtype=torch.int32, device="cuda")
	idx = torch.full((Q * k + 64,), -1, dtype=torch.int32, device="cuda")
	rc = lib.anncur_sparse_score_topk(p(q[0]), p(q[1]), p(q[2]), Q, p(post.term_ptr), p(post.post_item), p(post.post_val), post.n_terms, I, k,
									  val.data_ptr(), idx.data_ptr(), buf[off:].data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
	torch.cuda.synchronize()
	assert rc == 0, lib.anncur_last_error()
	_check_topk(ops, ops.TopK(val[:Q * k].view(torch.float32).view(Q, k), idx[:Q * k].view(Q, k)), ref, k, "C ABI top-k")
	assert (val[Q * k:] == -1).all() and (idx[Q * k:] == -1).all(), "guard behind an output"
	assert (buf[:off] == 0xff).all() and (buf[off + nbytes:] == 0xff).all(), "guard around the workspace"
	# a short workspace is refused before anything is written
	assert lib.anncur_sparse_score_topk(p(q[0]), p(q[1]), p(q[2]), Q, p(post.term_ptr), p(post.post_item), p(post.post_val), post.n_terms, I, k,
										val.data_ptr(), idx.data_ptr(), buf[off:].data_ptr(), nbytes - 4, None) == -2          # ANNCUR_E_WORKSPACE

