"""The index classes of anncur_amd/nearest_nbr.py -- k-means training, add, search -- held BIT FOR BIT to their host restatement,
tests/ivf_index_numpy.py (itself held by tests/test_cpu_ivf_index_reference.py).  No tolerance anywhere in this file.

Data are integers in [-8, 8]: sums of rows and inner products of two data vectors are exact in fp32 in any order, and a score against an fp32
centroid is the k-ordered fmaf chain of ops.gemm, restated in fp64 under a per-step TwoSum exactness check (a draw that fails it is replaced,
at most 5 times: ivf_index_numpy.exact_case).  n = 1500 .. 4096, d in {24, 64, 130}, nlist in {7, 16, 64}, three k-means iterations.
Every search runs on poisoned scratch (+inf over ops._ScoreScratch, 0xff over ops._ByteScratch), as in tests/test_gpu_ivf_exact.py.

ops.renorm_rows is compared first, alone: the correct rounding of 1.0f / sqrtf(x) on the device is what the rest builds on.

The bf16 FlatIPIndex orders ties by the ROW of its descending-norm packed copy (the header's contract for item_ids), which is the smaller
id only between vectors of one norm bucket: the test asserts the smaller id on equal-norm data and the row order on general data.

Mutations tried on scratch copies of nearest_nbr.py / ops.py when this file was written (Python only; 94 tests, 6.2 s on an MI355X); each is
named with the tests that fail on it, none survives:
  * renormalise BEFORE the split of empty lists: test_train_equals_..[prototypes-spherical] (the only case with splits), and 8 add / search
    tests on that index.
  * no renormalisation of the initial centroids: every spherical case of test_train_equals_.. (at niter = 0 already), 67 tests in all.
  * means taken from the NEXT list's rows (offsets shifted by one): all 9 cases of test_train_equals_.., 79 tests in all.
  * assignment ties to the LARGER list: test_train_equals_..[prototypes-*] (duplicate initial centroids) and [d24 / d64 / d130-plain] (integer
    initial centroids: integer scores tie); the spherical random cases have no exact ties and pass, as they should.
  * an unsorted sub-sample: test_train_equals_..[subsample-spherical], test_add_builds_the_reference_lists[subsample-*].
  * add() that keeps the lists of the first call: test_add_twice_equals_add_once[fp32, bf16].
  * the query pad left uninitialised (torch.empty for qp): 48 search tests -- every index whose rows are padded (d = 24, 130; d = 64 on bf16
    lists); d = 64 on fp32 lists has no pad and passes.  Caught because _search leaves NaN-filled freed blocks of qp's size with the allocator:
    the lists' pad columns are zero, so finite garbage in the query pad changes nothing.
  * the queries written to the LAST d columns of the padded row: 51 tests: every search on a padded index, search_device included.
  * the exclusion filter run on k instead of k + e_max candidates: all 18 cases of test_search_with_exclusions.
  * score_topk_dense scoring chunk 0's rows in every chunk: test_score_topk_dense_row_chunks.
Needs an MI355X."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_index_numpy as R  # noqa: E402
from test_gpu_ivf_exact import _poisoned  # noqa: E402
from oracle import gemm_chain as G  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


def _bits(a):
	a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
	assert a.dtype == np.float32
	return np.ascontiguousarray(a).view(np.int32)


def _same_f32(got, want, what):
	g, w = _bits(got), _bits(want)
	assert g.shape == w.shape, f"{what}: shape {g.shape}, want {w.shape}"
	if not np.array_equal(g, w):
		bad = np.argwhere(g != w)
		first = tuple(int(x) for x in bad[0])
		raise AssertionError(f"{what}: {len(bad)} of {g.size} fp32 values differ in their bits; first at {first}: got {g[first]:#x}, want {w[first]:#x}")


def _same_result(got, want, what):
	"""(D, I) against (D, I): the scores by their bits, the ids exactly; names the first differing query."""
	(gD, gI), (wD, wI) = got, want
	assert gD.dtype == wD.dtype == np.float32 and gI.dtype == wI.dtype and gD.shape == wD.shape and gI.shape == wI.shape, what
	bad = np.flatnonzero(((_bits(gD) != _bits(wD)) | (gI != wI)).any(axis=1))
	if bad.size:
		q = int(bad[0])
		raise AssertionError(f"{what}: {bad.size} of {gD.shape[0]} queries differ; first q={q}\n got  D={gD[q].tolist()}\n want D={wD[q].tolist()}\n got  I={gI[q].tolist()}\n want I={wI[q].tolist()}")


# ------------------------------------------------------------------ ops.renorm_rows alone (first: the rest builds on its rounding)
def _renorm_in_buffer(ops, gpu, M, pad=5):
	"""ops.renorm_rows on M as rows 1 .. r of a NaN-filled [r + 2 x d + pad] buffer -> (the rows afterwards, True if nothing else was written)."""
	r, d = M.shape
	buf = torch.full((r + 2, d + pad), NAN, dtype=torch.float32)
	buf[1:r + 1, :d] = torch.from_numpy(M)
	before = buf.clone()
	dev = buf.to(gpu)
	out = ops.renorm_rows(dev[1:r + 1, :d])
	assert out.data_ptr() == dev[1:r + 1, :d].data_ptr()
	after = dev.cpu()
	frame = torch.ones_like(buf, dtype=torch.bool)
	frame[1:r + 1, :d] = False
	return after[1:r + 1, :d].numpy(), torch.equal(after.view(torch.int32)[frame], before.view(torch.int32)[frame])


@pytest.mark.parametrize("d", [1, 63, 64, 65, 255, 256, 257, 600])
def test_renorm_rows_equals_the_reference(ops, gpu, d):
	"""One and two and three columns per thread, partial waves, a single lane.  Fixed-point grid rows (their fmaf steps beyond column 256 stay
	exact in fp64; redrawn otherwise) and, where a thread holds one column, normal deviates; a zero row; rows inside a NaN-filled padded buffer."""
	for attempt in range(R.MAX_ATTEMPTS):
		g = np.random.default_rng([d, attempt])
		M = G.grid(g, (12, d))
		if d <= 256: M[6:] = g.standard_normal((6, d)).astype(F32) * F32(3)
		M[2] = 0
		try:
			want = R.renorm_rows_ref(M)
		except R.InexactStep:
			continue
		break
	else:
		raise AssertionError("no draw meets the exactness precondition")
	got, frame_kept = _renorm_in_buffer(ops, gpu, M)
	_same_f32(got, want, f"renorm_rows d={d}")
	assert frame_kept, "renorm_rows wrote outside its rows (pad columns or neighbouring rows)"
	assert (got[2] == 0).all()


@pytest.mark.parametrize("d", [37, 300])
def test_renorm_rows_on_the_edge_rows(ops, gpu, d):
	"""All zero, a NaN, squares that underflow: unchanged.  Squares that overflow: zeros.  One inf: NaN there, zeros elsewhere.  (ivf_index_numpy.edge_rows)"""
	M, want = R.edge_rows(d)
	got, frame_kept = _renorm_in_buffer(ops, gpu, M)
	assert R.same_bits(got, want).all(), np.argwhere(~R.same_bits(got, want))[:5]
	assert R.same_bits(got, R.renorm_rows_ref(M)).all()
	assert np.array_equal(_bits(got[:3]), _bits(M[:3])), "a zero / NaN / underflowing row was touched"
	assert frame_kept


# ------------------------------------------------------------------ training
def _new_index(name, dtype="fp32", spherical=True, niter=R.NITER):
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	c = R.CASES[name]
	return IVFFlatIPIndex(c["d"], c["nlist"], niter=niter, spherical=spherical, dtype=dtype, max_points_per_centroid=c.get("max_points_per_centroid", 256))


TRAIN_CASES = [(name, sph) for name in ("d24", "d64", "d130", "prototypes") for sph in (True, False)] + [("subsample", True)]


@pytest.mark.parametrize("name,spherical", TRAIN_CASES, ids=[f"{n}-{'spherical' if s else 'plain'}" for n, s in TRAIN_CASES])
def test_train_equals_the_reference_after_every_iteration(ops, name, spherical):
	"""index.centroids after train with niter = 0, 1, 2, 3, bit for bit.  niter = 0 holds the (sorted) sub-sample, the permutation and the renormalised
	initial centroids; every further count one assignment (ties to the smaller list), list build, means, split of empty lists (prototypes: at least
	8 of 16 lists are empty in every iteration) and renormalisation after the split."""
	X, _, info = R.exact_case(name, spherical)
	for t in range(R.NITER + 1):
		index = _new_index(name, spherical=spherical, niter=t)
		index.train(X)
		assert index.is_trained and index.centroids.dtype == torch.float32
		_same_f32(index.centroids, info["history"][t], f"{name}: centroids after {t} iterations")


@pytest.mark.parametrize("kind", ["strided", "fortran", "float64"])
def test_train_takes_other_layouts_and_types(ops, kind):
	"""A view with a column stride, a column-major array and a float64 array of the same values train the same centroids."""
	X, C, _ = R.exact_case("d24")
	if kind == "strided":
		wide = np.full((X.shape[0], 2 * X.shape[1]), 99, dtype=F32)
		wide[:, ::2] = X
		Xin = wide[:, ::2]
		assert not Xin.flags.c_contiguous
	elif kind == "fortran":
		Xin = np.asfortranarray(X)
		assert not Xin.flags.c_contiguous
	else:
		Xin = X.astype(np.float64)
	index = _new_index("d24")
	index.train(Xin)
	_same_f32(index.centroids, C, f"d24 trained on a {kind} input")


# ------------------------------------------------------------------ add
_BUILT = {}


def _built(name, dtype):
	"""(index trained on and holding the case's vectors, integer queries): built once per (case, dtype), searched by many tests (which only
	set nprobe / batched_from / grouped_call)."""
	if (name, dtype) not in _BUILT:
		X, C, _ = R.exact_case(name)
		index = _new_index(name, dtype)
		index.train(X)
		index.add(X)
		_same_f32(index.centroids, C, f"{name}: centroids")
		_BUILT[(name, dtype)] = (index, R.exact_queries(name, C))
	return _BUILT[(name, dtype)]


def _assert_lists(index, name, dtype):
	X, C, info = R.exact_case(name)
	off, ids, sizes, Xs = info["add"]
	d = R.CASES[name]["d"]
	dp = -(-d // 128) * 128 if dtype == "bf16" else -(-d // 16) * 16
	assert index.ntotal == X.shape[0]
	assert index._offsets.dtype == torch.int32 and np.array_equal(index._offsets.cpu().numpy(), off)
	assert index._ids.dtype == torch.int32 and np.array_equal(index._ids.cpu().numpy(), ids)
	assert isinstance(index._sizes, np.ndarray) and index._sizes.dtype == np.int64 and np.array_equal(index._sizes, sizes)
	assert tuple(index._Xs.shape) == (X.shape[0], dp)
	_same_f32(index._Xs[:, :d], Xs, f"{name}: list-ordered rows")
	assert (_bits(index._Xs[:, d:]) == 0).all(), "pad columns of the list-ordered rows are not +0"
	if dtype == "bf16":
		assert index._Xs16.dtype == torch.bfloat16 and tuple(index._Xs16.shape) == (X.shape[0], dp)
		_same_f32(index._Xs16.float(), index._Xs, f"{name}: bf16 copy of the rows")      # (integers up to 8 are bf16 values)
	else:
		assert index._Xs16 is None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["d24", "d64", "d130", "prototypes", "subsample"])
def test_add_builds_the_reference_lists(ops, name, dtype):
	"""_offsets / _ids / _sizes are the stable counting sort of the chain assignment under the trained centroids; _Xs the rows in list order,
	zero padded to a multiple of 16 floats, or of 128 with a bf16 copy.  (subsample: trained on 128 rows, all 1500 added.)"""
	index, _ = _built(name, dtype)
	_assert_lists(index, name, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_add_twice_equals_add_once(ops, dtype):
	"""Two add() calls with two (unequal) parts: every list is rebuilt from all vectors, ids count on from the first part."""
	X, C, _ = R.exact_case("d130")
	once, _ = _built("d130", dtype)
	index = _new_index("d130", dtype)
	index.train(X)
	h = X.shape[0] // 2 + 37
	index.add(X[:h])
	assert index.ntotal == h and int(index._offsets[-1]) == h
	index.add(X[h:])
	_assert_lists(index, "d130", dtype)
	for a, b in ((index._offsets, once._offsets), (index._ids, once._ids), (index._Xs, once._Xs)):
		assert torch.equal(a, b)


# ------------------------------------------------------------------ search
ROUTES = ("scan", "grouped", "sequence")


def _set_route(ops, index, route, kc):
	"""Puts the index on a route -> the tie rule of the kernel that then serves a search for kc candidates.
	scan: fewer queries than batched_from, ivf_scan ("id").  grouped: the one-call search ("packed"), which hands over to ivf_scan_grouped
	("slotted") above IVF_GROUPED_MAX_K candidates.  sequence: grouped_call = False, ivf_scan_grouped ("slotted")."""
	index.batched_from = 256 if route == "scan" else 1
	index.grouped_call = route != "sequence"
	if route == "scan": return "id"
	return "packed" if route == "grouped" and ops.ivf_search_grouped_ok(kc, index.nlist) else "slotted"


def _want(name, Q, nprobe, k, ties, exclude=None):
	X, C, info = R.exact_case(name)
	off, ids, _, Xs = info["add"]
	return R.search_ref(Xs, off, ids, C, Q, nprobe, k, ties, exclude)


def _dirty_freed_memory(index, nq):
	"""Leaves NaN-filled blocks of the padded queries' size (fp32 and bf16) with the caching allocator: a query pad that the search allocates
	but does not zero then most likely holds NaN, not an earlier call's zeros."""
	dev = index.centroids.device
	blocks = [torch.full((nq, index._dp), NAN, dtype=dt, device=dev) for dt in (torch.float32, torch.bfloat16) for _ in range(2)]
	torch.cuda.synchronize()
	del blocks


def _search(ops, index, Q, k, exclude=None):
	def call():
		_dirty_freed_memory(index, Q.shape[0])
		return index.search(Q, k, exclude=exclude)
	return _poisoned(ops, call)


def _nprobes(nlist):
	return (1, int(math.floor(math.sqrt(nlist))), nlist, nlist + 5)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["d24", "d64", "d130", "prototypes"])
def test_search_equals_the_reference(ops, name, dtype, route):
	"""D and I for 40 queries, k = 10, nprobe = 1, floor(sqrt(nlist)), nlist and nlist + 5 (clamped to nlist), on every route.  d = 24 and 130 pad
	the queries (to 32 / 144 floats, 128 / 256 on a bf16 index), d = 64 does not on an fp32 index.  prototypes: 8 distinct vectors x 200, so every
	score ties 200-fold and the result IS the tie rule; half of its lists are empty."""
	index, Q = _built(name, dtype)
	ties = _set_route(ops, index, route, 10)
	for nprobe in _nprobes(index.nlist):
		index.nprobe = nprobe
		_same_result(_search(ops, index, Q, 10), _want(name, Q, nprobe, 10, ties), f"{name} {dtype} {route} nprobe={nprobe}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_search_pads_when_the_probed_lists_are_short(ops, dtype, route):
	"""nprobe = 1 on lists of about 64 vectors: k = 120 (still the one-call search) and k = 200 (above IVF_GROUPED_MAX_K: the one-call route hands
	over to ivf_scan_grouped) leave slots without a result: (-FLT_MAX, -1).  k = 200 with four probed lists is filled and cut inside a list."""
	index, Q = _built("d130", dtype)
	for k, nprobe in ((120, 1), (200, 1), (200, 4)):
		ties = _set_route(ops, index, route, k)
		assert ties == ("id" if route == "scan" else "packed" if route == "grouped" and k == 120 else "slotted")
		index.nprobe = nprobe
		want = _want("d130", Q, nprobe, k, ties)
		assert nprobe > 1 or ((want[1] == -1).any(axis=1).all() and (want[0][want[1] == -1] == np.finfo(F32).min).all())
		assert nprobe == 1 or (want[1][:, -1] >= 0).all()
		_same_result(_search(ops, index, Q, k), want, f"d130 {dtype} {route} k={k} nprobe={nprobe}")


def _exclusions(name, Q, nprobe, n):
	"""{kind: exclude argument}.  Built from the unfiltered result so that they bite: "shared" the best three of the first eight queries, one list
	for all; "per_query" every query's own best q % 5 and id q (lengths 1 .. 5); "long" 125 ids with those of "shared" among them: 135 candidates
	per query, above IVF_GROUPED_MAX_K."""
	_, I = _want(name, Q, nprobe, 10, "id")
	shared = sorted(set(int(i) for i in I[:8, :3].ravel() if i >= 0))
	per_query = [sorted(set([q] + [int(i) for i in I[q, :q % 5] if i >= 0])) for q in range(Q.shape[0])]
	more = [int(i) for i in np.random.default_rng(5).permutation(n) if int(i) not in shared]
	return {"shared": shared, "per_query": per_query, "long": sorted(shared + more[:125 - len(shared)])}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["shared", "per_query", "long"])
def test_search_with_exclusions(ops, gpu, kind, dtype, route):
	"""exclude= as one list and as one list per query: the search keeps k + the longest list candidates, the filter the first k allowed ones.
	search_device gives the same on the device ((-inf, -1) in empty slots, int32 ids)."""
	index, Q = _built("d130", dtype)
	index.nprobe = nprobe = 8
	excl = _exclusions("d130", Q, nprobe, index.ntotal)[kind]
	e_max = max(len(e) for e in excl) if kind == "per_query" else len(excl)
	assert e_max == (125 if kind == "long" else e_max) and e_max >= 3
	ties = _set_route(ops, index, route, 10 + e_max)
	want = _want("d130", Q, nprobe, 10, ties, excl)
	hit = set(excl) if kind != "per_query" else None
	assert all(not (set(want[1][q].tolist()) & (hit if hit is not None else set(excl[q]))) for q in range(Q.shape[0]))
	assert not np.array_equal(want[1], _want("d130", Q, nprobe, 10, ties)[1]), "the exclusion does not change the result"
	_same_result(_search(ops, index, Q, 10, excl), want, f"d130 {dtype} {route} exclude={kind}")
	qd = torch.from_numpy(Q).to(gpu)
	v, i = _poisoned(ops, lambda: (_dirty_freed_memory(index, Q.shape[0]), index.search_device(qd, 10, exclude=excl))[1])
	assert v.is_cuda and i.is_cuda and i.dtype == torch.int32
	_same_result((v.cpu().numpy(), i.cpu().numpy()), R.device_form(*want), f"d130 {dtype} {route} search_device exclude={kind}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_search_device_equals_the_reference(ops, gpu, dtype, route):
	"""Device-resident queries (d = 24: padded inside the call), no exclusion; k = 300 on nprobe = 1 pads with (-inf, -1)."""
	index, Q = _built("d24", dtype)
	qd = torch.from_numpy(Q).to(gpu)
	for k, nprobe in ((10, 2), (300, 1)):
		ties = _set_route(ops, index, route, k)
		index.nprobe = nprobe
		v, i = _poisoned(ops, lambda: (_dirty_freed_memory(index, Q.shape[0]), index.search_device(qd, k))[1])
		assert v.is_cuda and i.is_cuda and i.dtype == torch.int32 and v.dtype == torch.float32
		_same_result((v.cpu().numpy(), i.cpu().numpy()), R.device_form(*_want("d24", Q, nprobe, k, ties)), f"d24 {dtype} {route} search_device k={k}")


def test_build_flat_or_ivff_index_just_above_the_threshold(ops):
	"""11 001 vectors of d = 16: the IVF class with nlist = floor(sqrt(n)) = 104, nprobe = floor(sqrt(104)) = 10, the class defaults (10 iterations,
	seed 1234, no sub-sample: 104 * 256 > n) -- centroids, lists and one search against the reference; 11 000 vectors give the flat index."""
	from anncur_amd.nearest_nbr import FlatIPIndex, IVFFlatIPIndex, build_flat_or_ivff_index
	n, d = 11001, 16
	for attempt in range(R.MAX_ATTEMPTS):
		g = np.random.default_rng([11001, attempt])
		X, Q = g.integers(-8, 9, (n, d)).astype(F32), g.integers(-8, 9, (20, d)).astype(F32)
		try:
			C, info = R.train_ref(X, 104, 10)
			off, ids, sizes, Xs = R.add_ref(X, C)
			want = R.search_ref(Xs, off, ids, C, Q, 10, 10, "id")
		except R.InexactStep:
			continue
		break
	else:
		raise AssertionError("no draw meets the exactness precondition")
	assert info["subsampled"] is None
	index = build_flat_or_ivff_index(X, force_exact_search=False)
	assert type(index) is IVFFlatIPIndex and index.nlist == 104 and index.nprobe == 10 and index.ntotal == n and index.niter == 10 and index.dtype == "fp32"
	_same_f32(index.centroids, C, "centroids")
	assert np.array_equal(index._offsets.cpu().numpy(), off) and np.array_equal(index._ids.cpu().numpy(), ids)
	_same_result(_search(ops, index, Q, 10), want, "search")
	assert type(build_flat_or_ivff_index(X[:11000], force_exact_search=False)) is FlatIPIndex
	assert type(build_flat_or_ivff_index(X, force_exact_search=True)) is FlatIPIndex


# ------------------------------------------------------------------ FlatIPIndex
def _grid_problem():
	"""700 grid vectors of d = 70 (20 of them copies of earlier ones: ties), 33 grid queries; the chain differs from the once-rounded product here."""
	g = np.random.default_rng(70)
	X, Q = G.grid(g, (700, 70)), G.grid(g, (33, 70))
	X[500:520] = X[100:120]
	G.assert_exact_in_fp64(Q, X.T)
	S = R.chain_scores(Q, X.T)
	assert (S != G.once_rounded(Q, X.T)).mean() > 0.05 and (S != G.chain_reversed(Q, X.T)).mean() > 0.05
	return X, Q


def test_flat_fp32_equals_the_chain(ops):
	"""D = the chain's values, I breaks ties to the smaller id (copies 500 .. 519 come after their originals); add() in two parts; k above ntotal
	pads; exclude= shared and per query."""
	from anncur_amd.nearest_nbr import FlatIPIndex
	X, Q = _grid_problem()
	index = FlatIPIndex(70)
	index.add(X[:333])
	assert index.ntotal == 333
	index.add(X[333:])
	assert index.ntotal == 700
	want = R.flat_search_ref(X, Q, 10)
	_same_result(index.search(Q, 10), want, "flat fp32 k=10")
	both = [(int(a), int(b)) for row in R.flat_search_ref(X, Q, 700)[1] for a, b in zip(row[:-1], row[1:]) if a >= 100 and a < 120 and b == a + 400]
	assert len(both) >= 20 * 33 - 33, "the copies do not follow their originals in the reference"
	_same_result(index.search(Q, 700), R.flat_search_ref(X, Q, 700), "flat fp32 k = ntotal")
	shared = sorted(set(int(i) for i in want[1][:8, :3].ravel()))
	per_query = [sorted(set([q] + [int(i) for i in want[1][q, :q % 5]])) for q in range(Q.shape[0])]
	for what, excl in (("shared", shared), ("per query", per_query)):
		w = R.flat_search_ref(X, Q, 10, excl)
		assert not np.array_equal(w[1], want[1])
		_same_result(index.search(Q, 10, exclude=excl), w, f"flat fp32 exclude {what}")
	small = FlatIPIndex(70)
	small.add(X[:50])
	D, I = small.search(Q, 60)
	w = R.flat_search_ref(X[:50], Q, 60)
	assert (w[1][:, 50:] == -1).all() and (w[0][:, 50:] == np.finfo(F32).min).all() and (w[1][:, :50] >= 0).all()
	_same_result((D, I), w, "flat fp32 k above ntotal")


def test_score_topk_dense_row_chunks(ops, gpu):
	"""max_bytes = 3 rows of scores: 10 queries run as 3 + 3 + 3 + 1.  Equal to the unchunked call and to the reference, bit for bit."""
	X, Q = _grid_problem()
	Xd, Qd = torch.from_numpy(X).to(gpu), torch.from_numpy(Q[:10]).to(gpu)
	I = X.shape[0]
	assert [min(10, q0 + 3) - q0 for q0 in range(0, 10, max(1, min(10, (3 * 4 * I) // (4 * I))))] == [3, 3, 3, 1]
	whole = ops.score_topk_dense(Qd, Xd, 10)
	chunked = ops.score_topk_dense(Qd, Xd, 10, max_bytes=3 * 4 * I)
	assert torch.equal(chunked.values.view(torch.int32), whole.values.view(torch.int32)) and torch.equal(chunked.indices, whole.indices)
	D, Iw = R.flat_search_ref(X, Q[:10], 10)
	assert len(set(map(tuple, Iw.tolist()))) == 10, "the queries' results must differ for a misplaced chunk to show"
	_same_result((chunked.values.cpu().numpy(), chunked.indices.cpu().numpy().astype(np.int64)), (D, Iw), "score_topk_dense in chunks of 3")


def _int_scores_ranked(X, Q, k, rank):
	"""Exact integer scores, descending, ties to the smaller rank[id] -> (D, I) in FAISS' convention."""
	S = (Q.astype(np.float64) @ X.astype(np.float64).T)
	assert (S == np.rint(S)).all() and np.abs(S).max() < 1 << 24
	key = S.astype(np.int64) * (1 << 32) - rank[None, :].astype(np.int64)
	order = np.argsort(-key, axis=1, kind="stable")[:, :k]
	return np.take_along_axis(S, order, axis=1).astype(F32), order.astype(np.int64)


@pytest.mark.parametrize("norms", ["equal", "general", "small"])
def test_flat_bf16_on_integer_data(ops, norms):
	"""A bf16 index on bf16-exact data: the values are the exact integer scores.  9000 vectors take the fused score + top-k kernel.  equal: every
	vector is a signed permutation of one multiset, so all norms are equal, the descending-norm copy keeps the id order and ties go to the smaller
	id.  general: integers in [-8, 8]; ties go to the smaller ROW of the descending-norm copy (index._ids maps rows to ids; inside a norm bucket
	that is the smaller id, so copies still follow their originals).  small: 3000 vectors are too few for the fused kernel's sample; the index
	falls back to the fp32 route on its stored vectors: ties to the smaller id."""
	from anncur_amd.nearest_nbr import FlatIPIndex
	g = np.random.default_rng(64 + (norms == "equal"))
	n, d, nq, k = (3000 if norms == "small" else 9000), 64, 50, 10
	if norms == "equal":
		X = (g.permuted(np.tile(np.arange(d) % 9, (n, 1)), axis=1) * g.choice([-1, 1], (n, d))).astype(F32)
		assert np.unique((X * X).sum(axis=1)).size == 1
	else:
		X = g.integers(-8, 9, (n, d)).astype(F32)
	X[1000:1100] = X[0:100]
	Q = g.integers(-8, 9, (nq, d)).astype(F32)
	index = FlatIPIndex(d, dtype="bf16")
	index.add(X)
	kp = ops.padded_k(d)
	assert kp is not None and ops.fused_supported(nq, n, kp, k) == (norms != "small"), "the case left the route it was written for"
	got = index.search(Q, k)
	if norms == "small":
		assert index._Xp is None
		want = R.flat_search_ref(X, Q, k)
		assert (want[0][:, :-1] == want[0][:, 1:]).any(), "no ties among the results"
		_same_result(got, want, "flat bf16 index on the fp32 route")
		return
	assert index._Xp is not None and index._Xp.dtype == torch.bfloat16, "the fused route did not run"
	row_to_id = index._ids.cpu().numpy().astype(np.int64)
	assert np.array_equal(np.sort(row_to_id), np.arange(n))
	if norms == "equal":
		assert np.array_equal(row_to_id, np.arange(n))
	rank = np.empty(n, dtype=np.int64)
	rank[row_to_id] = np.arange(n)
	assert (rank[1000:1100] > rank[0:100]).all()
	want = _int_scores_ranked(X, Q, k, rank)
	assert (want[0][:, :-1] == want[0][:, 1:]).any(), "no ties among the results"
	_same_result(got, want, f"flat bf16, {norms} norms")
	if norms == "equal":
		_same_result(got, R.flat_search_ref(X, Q, k), "flat bf16 against the fp32 reference (ties to the smaller id)")
