"""`exclude=` through every retrieval route, on exact integer-valued data, against torch.topk on the CPU of the score matrix
with the excluded cells set to -inf.  Ids and values must be equal: no tolerance.

The data.  Query q reads two embedding columns of its own: X[q, 2q] = 64, X[q, 2q + 1] = 1, and item i holds there the two digits of a
code that is a permutation of range(I) per query: S[q, i] = 64 hi + lo with hi in [-128, 128), lo in [0, 64) -- distinct integers along
every row, every operand exact in bf16, every partial sum an integer below 2^24.  So a row has no ties and one right answer.  (The CUR
indexes are built over an identity anchor block, U = I; their anchor items score X[q, j] and do tie -- there the reference orders ties
by the smaller id, the library's documented order, which the filter keeps because it keeps the producer's order.)

Shapes: the smallest item counts the fused path takes for the k + e_max of the cases (found on the host with ops.fused_supported and
asserted below), plus a ragged tail; every test asserts the route it means to run.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, K_TOP, E_MAX = 33, 10, 16            # 33 queries: a ragged last workgroup of the filter (4 queries each) and a ragged 32-query sub-tile
I_256, I_WIDE = 8192 + 11, 4096 + 11    # smallest item counts of the Kp <= 512 bodies / the wide kernel, with a ragged tail
I_CUR = 13440 + 27                      # excluding 200 anchor items asks the Kp = 256 sweep for k + 200 candidates: it takes that from 13440 items
PAD = np.finfo(np.float32).min


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


# ------------------------------------------------------------------ data and reference
@functools.lru_cache(maxsize=None)
def _case(I, K, seed=0):
	"""(X [Q x K] float32, E [I x K] float32, S [Q x I] int64), computed once per shape and shared (never modified)."""
	assert K >= 2 * Q and I <= 256 * 64
	rng = np.random.default_rng(seed + I + K)
	code = np.stack([rng.permutation(I) for _ in range(Q)])                  # [Q x I]
	X = np.zeros((Q, K), dtype=np.float32)
	E = np.zeros((I, K), dtype=np.float32)
	q = np.arange(Q)
	X[q, 2 * q], X[q, 2 * q + 1] = 64, 1
	E[:, 0:2 * Q:2], E[:, 1:2 * Q:2] = (code // 64 - 128).T, (code % 64).T
	S = torch.from_numpy(X.astype(np.int64) @ E.astype(np.int64).T)
	assert all(np.unique(r).size == I for r in S.numpy())                    # tie-free rows
	return X, E, S


def _reference(S, k, excl_lists):
	"""torch.topk on the CPU of S (int64 [Q x I]) with the excluded cells at -inf; ties (the CUR anchor items only) by the smaller id.
	-> (values float32 [Q x k], ids int64 [Q x k])."""
	I = S.shape[1]
	Sf = S.double().clone()
	for q, ids in enumerate(excl_lists):
		if len(ids): Sf[q, torch.as_tensor(np.asarray(ids, dtype=np.int64))] = -np.inf
	key = Sf * (1 << 14) - torch.arange(I, dtype=torch.float64)              # |S| < 2^14, I < 2^14: exact in fp64; -inf stays -inf
	ids = torch.topk(key, k, dim=1).indices
	vals = torch.gather(Sf, 1, ids)
	assert torch.isfinite(vals).all()
	return vals.float().numpy(), ids.numpy()


def _exclusions(S, k, e, seed):
	"""The four cases of the issue as lists of Q lists (None: shared) -> {name: (exclude argument, per-query lists for the reference)}."""
	rng = np.random.default_rng(seed)
	I = S.shape[1]
	own = [list(map(int, r)) for r in torch.topk(S.double(), e, dim=1).indices.numpy()]    # every leading candidate goes
	rand = [list(map(int, rng.permutation(I)[:rng.integers(0, e + 1)])) for _ in range(Q)]
	rand[0] = rand[0] + rand[0][:2]                                                          # duplicates, unsorted
	shared = list(map(int, rng.permutation(I)[:e]))
	shared[:3] = own[1][:3]                                                                  # ... and it removes something from query 1
	mixed = [own[q] if q % 2 else [] for q in range(Q)]
	padded = np.full((Q, e), -1, dtype=np.int64)                                             # the 2-D form of `rand`
	for q, r in enumerate(rand): padded[q, :len(set(r))] = sorted(set(r))
	return {"own_top_e": (own, own), "random": (rand, rand), "random_2d": (padded, rand), "shared": (np.asarray(shared), [shared] * Q), "mixed": (mixed, mixed)}


def _assert_equal(D, Idx, want_v, want_i, what):
	Idx = np.asarray(Idx).astype(np.int64)
	bad = np.nonzero((Idx != want_i).any(1) | (np.asarray(D, dtype=np.float32) != want_v).any(1))[0]
	assert bad.size == 0, f"{what}: {bad.size} queries differ, first q={bad[0]}\n got  {Idx[bad[0]]}\n want {want_i[bad[0]]}\n got  {np.asarray(D)[bad[0]]}\n want {want_v[bad[0]]}"


# ------------------------------------------------------------------ FlatIPIndex: the three routes through the public call
FLAT_ROUTES = {  # name -> (index dtype, K, I, Kp of the fused operands or None)
	"bf16-256": ("bf16", 200, I_256, 256), "bf16-wide": ("bf16", 600, I_WIDE, 640),
	"fp32-dense": ("fp32", 200, I_256, None),
	"bf16x3-256": ("bf16x3", 80, I_256, 256), "bf16x3-wide": ("bf16x3", 200, I_WIDE, 640),
}


@functools.lru_cache(maxsize=None)
def _flat_index(route):
	from anncur_amd.nearest_nbr import FlatIPIndex
	dtype, K, I, _ = FLAT_ROUTES[route]
	X, E, S = _case(I, K)
	index = FlatIPIndex(K, dtype=dtype)
	index.add(E)
	return index, X, S


def _assert_route(ops, route, index, kc_sweep):
	"""The route the case is written for: asserted from the plan queries before, and from what the index built after the search."""
	dtype, K, I, Kp = FLAT_ROUTES[route]
	if dtype == "fp32":
		assert index._Xp is None and index._split is None                    # neither fused operand was ever packed: the dense fp32 route
		return
	assert (ops.padded_k(K) if dtype == "bf16" else ops.split_kp(K)) == Kp
	assert ops.fused_supported(Q, I, Kp, kc_sweep), "the case left the fused path"
	assert not ops.fused_supported(Q, I - 11 - 64, Kp, kc_sweep), "a smaller item count would do"
	assert (ops.fused_plan(Q, I, Kp, kc_sweep)["lg"] == 4) == (Kp > 512)      # the wide kernel / a register-resident body
	if dtype == "bf16":
		assert index._Xp is not None and index._Xp.shape[1] == Kp            # packed at the first fused search only
	else:
		assert index._split is not None and index._split.kp == Kp


@pytest.mark.parametrize("route", list(FLAT_ROUTES))
def test_flat_index_exclusion_cases(ops, route):
	index, X, S = _flat_index(route)
	dtype, K, I, Kp = FLAT_ROUTES[route]
	k, e = K_TOP, E_MAX
	for name, (arg, lists) in _exclusions(S, k, e, seed=len(route)).items():
		want_v, want_i = _reference(S, k, lists)
		D, Idx = index.search(X, k, exclude=arg)
		assert D.dtype == np.float32 and Idx.dtype == np.int64 and D.shape == Idx.shape == (Q, k)
		_assert_equal(D, Idx, want_v, want_i, f"{route} {name}")
	e_used = ops.exclusion(_exclusions(S, k, e, seed=len(route))["own_top_e"][0], Q, I, "cuda").e_max
	assert e_used == e
	if dtype == "bf16x3":
		excl = ops.exclusion(_exclusions(S, k, e, seed=len(route))["own_top_e"][0], Q, I, "cuda")
		assert index._split.takes(Q, I, k, excl)
		_assert_route(ops, route, index, ops.split_candidates(I, k, n_excl=e))
	else:
		_assert_route(ops, route, index, k + e)


@pytest.mark.parametrize("route", list(FLAT_ROUTES))
def test_flat_index_no_exclusion_is_bit_equal_to_the_plain_call(ops, route):
	index, X, S = _flat_index(route)
	plain = index.search(X, K_TOP)
	want_v, want_i = _reference(S, K_TOP, [[]] * Q)
	_assert_equal(plain[0], plain[1], want_v, want_i, f"{route} plain")
	for nothing in (None, [[]] * Q, [], np.full((Q, 4), -1)):
		got = index.search(X, K_TOP, exclude=nothing)
		assert np.array_equal(got[0].view(np.int32), plain[0].view(np.int32)) and np.array_equal(got[1], plain[1])


def test_flat_index_over_the_limit_raises(ops):
	"""FlatIPIndex.search uses k_eff = min(k, ntotal): fewer than k allowed items in the whole index means k_eff + e_max > ntotal, which is
	over the limit (the (-FLT_MAX, -1) padding is an IVF matter, tested below)."""
	from anncur_amd.nearest_nbr import FlatIPIndex
	X, E, _ = _case(I_256, 80)
	for dtype in ("fp32", "bf16", "bf16x3"):
		index = FlatIPIndex(80, dtype=dtype)
		index.add(E[:20])
		with pytest.raises(ValueError, match=r"10 \+ 11 = 21 .*min\(20, 2048\) = 20.*rebuild the index without those items"):
			index.search(X, 10, exclude=list(range(11)))
		with pytest.raises(ValueError, match=r"20 \+ 1 = 21"):
			index.search(X, 30, exclude=[[3]] + [[]] * (Q - 1))             # k_eff = 20
		with pytest.raises(ValueError, match="only 20 items"):
			index.search(X, 5, exclude=[20])
		D, Idx = index.search(X, 10, exclude=list(range(10)))               # 10 + 10 = 20: at the limit
		assert (Idx >= 10).all() and all(np.unique(r).size == 10 for r in Idx)
	big = _flat_index("bf16-256")[0]
	with pytest.raises(ValueError, match=r"min\(8203, 2048\) = 2048"):
		big.search(_flat_index("bf16-256")[1], 10, exclude=list(range(2039)))


# ------------------------------------------------------------------ the CUR indexes
def _cur_case(K, I):
	"""Anchor rows R = E^T [K x I] with an identity anchor block: R[:, anc] = 1, so U = pinv(1) = 1 and the index' E^T is R^T itself."""
	X, E, _ = _case(I, K)
	rng = np.random.default_rng(K)
	anc = np.sort(rng.choice(I, K, replace=False))
	R = E.T.copy()
	R[:, anc] = np.eye(K, dtype=np.float32)
	S = torch.from_numpy(X.astype(np.int64) @ R.astype(np.int64))
	return X, R, anc, S


@pytest.mark.parametrize("compute_dtype,K", [("bf16", 200), ("fp32", 80), ("bf16x3", 80)])
def test_cur_indexes_exclude_anchor_items_and_own_top_e(ops, compute_dtype, K):
	"""CURRowIndex.topk, CURApprox.topk_in_row and topk_in_row_device with exclude = the anchor items (the use the argument exists for:
	the caller holds their exact scores) as a cached Exclusion, and with each query's own top-e."""
	from anncur_amd.cur import CURApprox, CURRowIndex
	I, k, e = I_CUR, K_TOP, E_MAX
	X, R, anc, S = _cur_case(K, I)
	Rd = torch.from_numpy(R).cuda()
	if compute_dtype == "bf16": Rd = Rd.bfloat16()
	Xd = torch.from_numpy(X).cuda()
	row = CURRowIndex(Rd, anc, compute_dtype=compute_dtype, pinv_backend="numpy")
	assert torch.equal(row._Et.float().cpu(), torch.from_numpy(R.T.copy())), "the case needs U = identity exactly"
	full = CURApprox(rows=Rd, cols=torch.eye(K, device="cuda", dtype=Rd.dtype), row_idxs=np.arange(K), col_idxs=anc, approx_preference="rows",
					 compute_dtype=compute_dtype, pinv_backend="numpy")
	assert torch.equal(full._Et, row._Et)
	own = [list(map(int, r)) for r in _reference(S, e, [[]] * Q)[1]]
	anchors = ops.exclusion(anc, Q, I, "cuda")                                 # normalised once, reused by every call
	assert anchors.e_max == K and anchors.off is None
	for name, arg, lists in (("anchors", anchors, [list(anc)] * Q), ("own_top_e", own, own)):
		want_v, want_i = _reference(S, k, lists)
		em = K if name == "anchors" else e
		# the route
		if compute_dtype == "bf16":
			assert row._Etp is not None and ops.fused_supported(Q, I, row._Etp.shape[1], k + em)
		elif compute_dtype == "bf16x3":
			assert row._split.takes(Q, I, k, ops.exclusion(arg, Q, I, "cuda"))
		else:
			assert row._Etp is None and row._split is None
		got = row.topk(Xd if compute_dtype != "bf16" else Xd.bfloat16(), k, exclude=arg)
		assert got.values.is_cuda and got.indices.dtype == torch.int32
		_assert_equal(got.values.cpu().numpy(), got.indices.cpu().numpy(), want_v, want_i, f"CURRowIndex {compute_dtype} {name}")
		got = full.topk_in_row_device(Xd, k, exclude=arg)
		_assert_equal(got.values.cpu().numpy(), got.indices.cpu().numpy(), want_v, want_i, f"CURApprox device {compute_dtype} {name}")
		got = full.topk_in_row(torch.from_numpy(X), k, exclude=arg)            # CPU in -> CPU out, int64 ids
		assert not got.values.is_cuda and got.indices.dtype == torch.int64
		_assert_equal(got.values.numpy(), got.indices.numpy(), want_v, want_i, f"CURApprox {compute_dtype} {name}")
	# nothing to exclude: bit-equal to the call without the argument
	plain = row.topk(Xd if compute_dtype != "bf16" else Xd.bfloat16(), k)
	for nothing in (None, [[]] * Q):
		got = row.topk(Xd if compute_dtype != "bf16" else Xd.bfloat16(), k, exclude=nothing)
		assert torch.equal(got.values, plain.values) and torch.equal(got.indices, plain.indices)
		got = full.topk_in_row_device(Xd, k, exclude=nothing)
		assert torch.equal(got.values, plain.values) and torch.equal(got.indices, plain.indices)
	with pytest.raises(ValueError, match="rebuild the index"):
		row.topk(Xd if compute_dtype != "bf16" else Xd.bfloat16(), 2000, exclude=anchors)


# ------------------------------------------------------------------ IVFFlatIPIndex
IVF_D, IVF_NLIST, IVF_NQ = 16, 8, 300
IVF_SIZES = [150, 90, 64, 129, 70, 33, 5, 3]     # lists 6 and 7 together hold 8 vectors: fewer than k = 10


@functools.lru_cache(maxsize=None)
def _ivf_case():
	"""A hand-made inverted file on integer data.  Centroid l = 8 e_l; vector i of list l has x[l] = 1 (so it is assigned to l), and the two
	digits of a unique code in dimensions 8, 9; query q holds a permutation of 0..7 in dimensions 0..7 -- its centroid scores 8 perm[l] are
	distinct: the nprobe lists are known -- and (512, 8) or (-512, -8) in dimensions 8, 9: S[q, i] = +-8 code_i + perm_q[list_i], tie-free."""
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	rng = np.random.default_rng(11)
	n = sum(IVF_SIZES)
	lst = rng.permutation(np.repeat(np.arange(IVF_NLIST), IVF_SIZES))
	code = rng.permutation(n)
	Xv = np.zeros((n, IVF_D), dtype=np.float32)
	Xv[np.arange(n), lst] = 1
	Xv[:, 8], Xv[:, 9] = code // 64 - 4, code % 64
	perm = np.stack([rng.permutation(IVF_NLIST) for _ in range(IVF_NQ)])
	perm[0] = [0, 1, 2, 3, 4, 5, 7, 6]                                           # query 0 probes the two short lists
	Qv = np.zeros((IVF_NQ, IVF_D), dtype=np.float32)
	Qv[:, :IVF_NLIST] = perm
	sign = np.where(rng.random(IVF_NQ) < 0.5, -1, 1)
	Qv[:, 8], Qv[:, 9] = 512 * sign, 8 * sign
	index = IVFFlatIPIndex(IVF_D, IVF_NLIST)
	index.centroids = torch.from_numpy(8 * np.eye(IVF_NLIST, IVF_D, dtype=np.float32)).cuda()
	index.is_trained = True
	index.add(Xv)
	assert np.array_equal(index._sizes, np.asarray(IVF_SIZES))
	S = Qv.astype(np.int64) @ Xv.astype(np.int64).T
	return index, Qv, lst, perm, S


def _ivf_reference(S, lst, perm, nprobe, k, excl_lists):
	"""Brute force over the probed lists minus the excluded ids; (-FLT_MAX, -1) where fewer than k are left."""
	nq = S.shape[0]
	D = np.full((nq, k), PAD, dtype=np.float32)
	Idx = np.full((nq, k), -1, dtype=np.int64)
	for q in range(nq):
		probed = np.argsort(-perm[q])[:nprobe]
		cand = np.nonzero(np.isin(lst, probed))[0]
		cand = cand[~np.isin(cand, np.asarray(excl_lists[q], dtype=np.int64))]
		s = S[q, cand]
		assert np.unique(s).size == s.size
		o = np.argsort(-s)[:k]
		D[q, :o.size], Idx[q, :o.size] = s[o], cand[o]
	return D, Idx


@pytest.mark.parametrize("path", ["grouped_call", "scan_grouped", "per_query"])
def test_ivf_index_exclusion_against_brute_force_over_the_probed_lists(ops, path):
	"""grouped_call: the one-call search (k + e_max <= IVF_GROUPED_MAX_K); scan_grouped: k + e_max above that cap, served by the older batched
	path; per_query: fewer queries than batched_from.  Query 0 probes lists that hold 8 vectors in all, and loses 3 of them."""
	index, Qv, lst, perm, S = _ivf_case()
	index.nprobe = 2
	k, e = (100, 40) if path == "scan_grouped" else (10, 6)
	index.batched_from = 10 ** 9 if path == "per_query" else 256
	nq = 40 if path == "per_query" else IVF_NQ
	assert (nq >= index.batched_from) == (path != "per_query")
	assert index.grouped_call and (path == "per_query" or ops.ivf_search_grouped_ok(k + e, IVF_NLIST) == (path == "grouped_call"))
	plain_D, plain_I = index.search(Qv[:nq], k)
	want = _ivf_reference(S[:nq], lst, perm, 2, k, [[]] * nq)
	_assert_equal(plain_D, plain_I, want[0], want[1], f"{path} plain")
	own = [list(map(int, r[r >= 0][:e])) for r in plain_I]                     # each query's own leading results
	own[0] = own[0][:3]
	rng = np.random.default_rng(3)
	rand = [list(map(int, rng.permutation(len(lst))[:rng.integers(0, e + 1)])) for _ in range(nq)]
	shared = list(map(int, rng.permutation(len(lst))[:e]))
	cases = {"own": (own, own), "random": (rand, rand), "shared": (shared, [shared] * nq), "mixed": ([own[q] if q % 2 == 0 else [] for q in range(nq)],) * 2}
	for name, (arg, lists) in cases.items():
		want_D, want_I = _ivf_reference(S[:nq], lst, perm, 2, k, lists)
		D, Idx = index.search(Qv[:nq], k, exclude=arg)
		_assert_equal(D, Idx, want_D, want_I, f"{path} {name}")
		if name in ("own", "mixed"):
			assert (want_I[0, :5] >= 0).all() and (want_I[0, 5:] == -1).all() and (D[0, 5:] == PAD).all()   # 8 probed vectors, 3 excluded
	for nothing in (None, [[]] * nq):
		D, Idx = index.search(Qv[:nq], k, exclude=nothing)
		assert np.array_equal(D.view(np.int32), plain_D.view(np.int32)) and np.array_equal(Idx, plain_I)
	v, i = index.search_device(torch.from_numpy(Qv[:nq]).cuda(), k, exclude=own)
	want_D, want_I = _ivf_reference(S[:nq], lst, perm, 2, k, own)
	assert np.array_equal(i.cpu().numpy(), want_I) and np.array_equal(np.where(want_I >= 0, v.cpu().numpy(), PAD), want_D)
