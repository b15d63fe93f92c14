"""Exact-data tests of the inverted-file search (csrc/ivf.hip) against plain numpy on the host.

Vectors and queries are small integers ([-8, 8], d <= 512) stored as bf16 or fp32: every inner product is an integer of magnitude at most
64 * 512 = 32768 < 2^24, exact in fp32 under any accumulation order, on the matrix cores or not.  So nothing here has a tolerance: values
must be bit-equal to the integer reference cast to fp32, and the ids are deterministic as well because score ties have a defined winner
(the packed search and the round-4 pipeline: the smaller column of the query's row, i.e. probe-slot order, then list order; the per-query
scan: the smaller vector id, the key of select.hpp).  Narrow value ranges make ties the common case.

Every search call runs on POISONED scratch: ops._ScoreScratch is filled with +inf and ops._ByteScratch with 0xff bytes first, over their
whole size.  Both are grow-only and reused, the packed score matrix is never pre-filled, and the suite (like the benchmark's warm-up)
repeats searches -- without the poison a lost tile, a dropped tile row or a missed ragged edge replays the previous call's correct score;
with it the unwritten +inf wins the top-k and the comparison fails.

The builder kernels (ivf_build_lists, ivf_list_means, norm_buckets + descending_norm_order, ivf_map_ids) are compared with host
restatements: integer work exactly, the means within a derived 2^-22.

Mutations tried on scratch builds when this file was written (73 tests, 6.5 s on an MI355X next to 229 s for the rest of the GPU suite):
  * ivf_tile_desc_kernel never emits the last vector tile of a list (the one before it is computed twice): every tile128 case fails (12 tests).
    With the poison switched off and each call preceded by the same call on the correct library -- the state a repeated search leaves -- all
    of them PASS: the stale scores are the right ones.  That is the gap the poison closes.  (Unpoisoned on fresh memory they fail by luck.)
  * ops.ivf_search_grouped under-counts max_tiles by one: caught where the bound is tight (one or two lists, three tiles).
  * ivf_map_ids_packed_kernel with `c <= co + sz`: 22 of the 25 search tests run against it fail (ids).
  * ops.ivf_search_grouped slices probe but not Q per chunk: all of test_query_chunks fails.
  * the wave-select keys prefer the LARGER column on ties: all 19 tests run against it fail.
  * ivf_fill_kernel with a quarter length that is not rounded to 64: SURVIVES, and should -- both of its loops stop at `i < end`, so a wave
    step that straddles a quarter boundary drops the other quarter's lanes; the rounding only aligns the reads.  An equivalent mutant.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_index_numpy import lists_search_ref  # noqa: E402

pytestmark = pytest.mark.gpu
# Deterministic by default (the same examples every run); ANNCUR_FUZZ=1 draws fresh ones and ANNCUR_FUZZ_EXAMPLES=n draws more.
_FUZZ = os.environ.get("ANNCUR_FUZZ", "") not in ("", "0")
_N = int(os.environ.get("ANNCUR_FUZZ_EXAMPLES", "0"))

INF = float("inf")


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


# ------------------------------------------------------------------ the poison
def _scratch_state(ops):
	return sorted((cls.__name__, key, buf.data_ptr(), buf.numel()) for cls in (ops._ScoreScratch, ops._ByteScratch) for key, buf in cls._bufs.items())


def _poison(ops):
	"""+inf over the whole score scratch, 0xff over the whole byte workspace (all of each grow-only buffer, not only the part the next call takes)."""
	for buf in ops._ScoreScratch._bufs.values(): buf.fill_(INF)
	for buf in ops._ByteScratch._bufs.values(): buf.fill_(0xff)


def _poisoned(ops, call):
	"""call() on poisoned scratch.  A call that had to grow a buffer ran on fresh, unpoisoned memory: it is run again, now on the grown buffer
	poisoned over its whole size -- the sizes are the call's own, nothing of ops' sizing is restated here."""
	for _ in range(3):
		_poison(ops)
		before = _scratch_state(ops)
		out = call()
		torch.cuda.synchronize()
		if _scratch_state(ops) == before:
			return out
	raise AssertionError("the scratch buffers keep changing between identical calls")


# ------------------------------------------------------------------ the host reference
# (moved to tests/ivf_index_numpy.py, where the index classes' host restatement shares it; unchanged)
_reference = lists_search_ref


def _equal(got, want, what):
	"""torch.equal on the values AND on the ids; on a mismatch, name the first differing query."""
	gv, gi = got.values.cpu(), got.indices.cpu().to(torch.int32)
	wv, wi = torch.from_numpy(want[0]), torch.from_numpy(want[1])
	if torch.equal(gv, wv) and torch.equal(gi, wi): return
	bad = ((gv != wv) | (gi != wi)).any(dim=1).nonzero()[:, 0]
	q = int(bad[0])
	raise AssertionError(f"{what}: {bad.numel()} of {gv.shape[0]} queries differ; first q={q}\n got  v={gv[q].tolist()}\n want v={wv[q].tolist()}\n got  i={gi[q].tolist()}\n want i={wi[q].tolist()}")


def _padded(a, ld, dtype, device, fill=5):
	"""The integer matrix `a` as the [:, :d] view of a [rows x ld] tensor whose padding columns hold `fill` (a kernel that reads past d is wrong)."""
	buf = torch.full((a.shape[0], ld), float(fill), dtype=dtype)
	buf[:, :a.shape[1]] = torch.from_numpy(a).to(dtype)
	return buf.to(device)[:, :a.shape[1]]


def _check(ops, dev, sizes, probe, dp, dtype, k, vr=8, padx=0, padq=0, seed=0, old_paths=True, max_bytes=None):
	"""One problem on hand-built lists through ops.ivf_search_grouped (route asserted) and -- on valid probes -- through ops.ivf_scan_grouped
	(fp32 lists and bf16 lists) and ops.ivf_scan, each on poisoned scratch, each against the host reference (never against each other)."""
	from anncur_amd import _lib
	g = np.random.default_rng(seed)
	sizes = np.asarray(sizes, dtype=np.int64)
	probe = np.ascontiguousarray(probe, dtype=np.int32)
	nlist, (nq, nprobe) = sizes.shape[0], probe.shape
	n = max(int(sizes.sum()), 1)                                  # (the last list ends exactly at the end of Xs whenever any list has a vector)
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X = g.integers(-vr, vr + 1, (n, dp)).astype(np.int64)
	Q = g.integers(-vr, vr + 1, (nq, dp)).astype(np.int64)
	off_d, ids_d = torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev)
	kw = {} if max_bytes is None else {"max_bytes": max_bytes}

	Xd, Qd = _padded(X, dp + padx, dtype, dev), _padded(Q, dp + padq, dtype, dev)
	want_tile = 128 if dtype == torch.bfloat16 and dp % 128 == 0 else 64
	assert _lib.load().anncur_ivf_search_tile(ops._dt(Xd), dp, ops._ld(Xd), ops._ld(Qd), nq) == want_tile, "the case left the tile kernel it was written for"
	want = _reference(X, Q, off, ids, probe, k, ("packed",))["packed"]
	probe_d = torch.from_numpy(probe).to(dev)
	got = _poisoned(ops, lambda: ops.ivf_search_grouped(Xd, off_d, ids_d, sizes, Qd, probe_d, k, **kw))
	_equal(got, want, f"ivf_search_grouped tile{want_tile}")
	if max_bytes is not None:   # (second assertion of the chunked cases: the unchunked call gives the same bits)
		whole = _poisoned(ops, lambda: ops.ivf_search_grouped(Xd, off_d, ids_d, sizes, Qd, probe_d, k))
		assert torch.equal(got.values, whole.values) and torch.equal(got.indices, whole.indices)
	if not old_paths: return

	# the older paths do not skip invalid probes (ivf_scan_grouped clamps them to list 0): valid list ids only, put where the invalid ones were
	valid = (probe >= 0) & (probe < nlist)
	pv = np.where(valid, probe, (np.arange(nq)[:, None] + np.arange(nprobe)[None, :]) % nlist).astype(np.int32)
	lmax = -(-max(int(sizes.max()), 1) // 8) * 8
	want = _reference(X, Q, off, ids, pv, k, ("slotted",), lmax)["slotted"]
	pv_d = torch.from_numpy(pv).to(dev)
	Xf, Qf = _padded(X, dp + padx, torch.float32, dev), _padded(Q, dp + padq, torch.float32, dev)
	Xb = _padded(X, dp + padx, torch.bfloat16, dev)
	got = _poisoned(ops, lambda: ops.ivf_scan_grouped(Xf, off_d, ids_d, sizes, Qf, pv_d, k, **kw))
	_equal(got, want, "ivf_scan_grouped fp32")
	if max_bytes is not None:
		whole = _poisoned(ops, lambda: ops.ivf_scan_grouped(Xf, off_d, ids_d, sizes, Qf, pv_d, k))
		assert torch.equal(got.values, whole.values) and torch.equal(got.indices, whole.indices)
	got = _poisoned(ops, lambda: ops.ivf_scan_grouped(Xf, off_d, ids_d, sizes, Qf, pv_d, k, lists_bf16=Xb, **kw))
	_equal(got, want, "ivf_scan_grouped bf16 lists")
	# the per-query scan selects on (score, vector id) keys, distinct per row: a list is offered once (ivf_scan skips a probe of -1)
	ps = pv.copy()
	for s in range(1, nprobe):
		ps[(ps[:, s:s + 1] == ps[:, :s]).any(axis=1), s] = -1
	want = _reference(X, Q, off, ids, ps, k, ("id",))["id"]
	ps_d = torch.from_numpy(ps).to(dev)
	got = ops.ivf_scan(Xf, off_d, ids_d, Qf, ps_d, k)
	_equal(got, want, "ivf_scan")


def _random_probe(g, nq, nprobe, nlist, invalid=0.0):
	"""Random probe rows (a list may appear twice in a row); a fraction `invalid` of the entries are -1 or ids at / past nlist."""
	probe = g.integers(0, nlist, (nq, nprobe))
	m = g.random((nq, nprobe))
	probe[m < invalid / 2] = -1
	probe[(m >= invalid / 2) & (m < invalid)] = nlist + g.integers(0, 3)
	return probe.astype(np.int32)


EDGE_SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 0, 3000, 2, 1, 3]   # list sizes around the 64- and 128-vector tile edges, one long list

BF16, F32 = torch.bfloat16, torch.float32
ROUTES = [(BF16, 128), (BF16, 256), (BF16, 384), (BF16, 512),   # 128 x 128 tiles: one, two, three, four pairs of k-tiles
		  (BF16, 16), (BF16, 80), (BF16, 192),                  # 64 x 64 bf16 tiles
		  (F32, 16), (F32, 48), (F32, 208)]                     # 64 x 64 fp32 tiles
_route_id = lambda r: f"{'bf16' if r[0] == BF16 else 'fp32'}-{r[1]}"
THREE = [(BF16, 128), (BF16, 80), (F32, 48)]                    # one case per tile kernel


# ------------------------------------------------------------------ A. the grouped search on exact data
@pytest.mark.parametrize("route", ROUTES, ids=_route_id)
def test_routes_on_list_sizes_around_the_tile_edges(ops, gpu, route):
	"""Every route on lists of 0, 1, 63 .. 257 and 3000 vectors, padded ldx / ldq (row-padded tensors, sliced; 16-byte contract kept), probes
	with -1 and out-of-range entries, narrow values on half the routes (ties everywhere)."""
	dtype, dp = route
	i = ROUTES.index(route)
	g = np.random.default_rng(100 + i)
	probe = _random_probe(g, 257, 5, len(EDGE_SIZES), invalid=0.15)
	probe[0] = [12, 10, 9, 8, 7]                                 # the long list first, then 257, 256, 255, 129
	probe[1] = [0, 11, 0, 11, -1]                                # only empty lists
	_check(ops, gpu, EDGE_SIZES, probe, dp, dtype, k=(1, 10, 64, 128)[i % 4], vr=(8, 1, 2)[i % 3], padx=(0, 8, 24)[i % 3], padq=(16, 0, 8)[i % 3], seed=i)


@pytest.mark.parametrize("route", THREE, ids=_route_id)
def test_pairs_per_list_around_the_tile_edges(ops, gpu, route):
	"""Lists probed by exactly 0, 1, 63, 64, 65, 127, 128, 129 and 300 (= all) queries: the pair tiles' ragged edges for both tile sizes."""
	dtype, dp = route
	sizes = [130, 5, 64, 129, 70, 33, 0, 77, 65, 64, 63, 200]
	nq = 300
	probe = np.full((nq, 10), -1, dtype=np.int32)
	q = np.arange(nq)
	probe[:, 0] = 0                                               # list 0: all 300 queries
	probe[7, 1] = 1                                               # list 1: one query
	probe[q < 127, 2] = 2
	probe[(q >= 100) & (q < 228), 3] = 3                          # 128
	probe[q >= nq - 129, 4] = 4                                   # 129; list 5: nobody
	probe[:, 5] = np.where(q % 2 == 0, 6, 7)                      # an empty list for the even queries
	probe[q < 63, 6] = 8
	probe[(q >= 10) & (q < 74), 7] = 9                            # 64
	probe[q % 4 == 1, 8] = 10; probe[q >= 4 * 65, 8] = -1         # 65 (q = 1, 5, .. 257)
	probe[q < 3, 9] = 11
	for l, c in ((0, 300), (1, 1), (2, 127), (3, 128), (4, 129), (5, 0), (8, 63), (9, 64), (10, 65)):
		assert int((probe == l).sum()) == c
	_check(ops, gpu, sizes, probe, dp, dtype, k=64, vr=2, seed=7)


@pytest.mark.parametrize("route", [(BF16, 256), (F32, 16)], ids=_route_id)
def test_all_queries_probe_the_same_lists(ops, gpu, route):
	"""1000 queries, all on the same three lists: every list gets nq pairs, many pair tiles times many vector tiles."""
	dtype, dp = route
	probe = np.tile(np.array([2, 0, 1], dtype=np.int32), (1000, 1))
	_check(ops, gpu, [257, 1000, 64, 9], probe, dp, dtype, k=64, vr=8, padx=8, padq=8, seed=11)


@pytest.mark.parametrize("nq,nlist,k,route", [(1, 1, 1, (BF16, 128)), (2, 2, 10, (F32, 48)), (255, 257, 64, (BF16, 80)), (256, 1000, 128, (BF16, 128)),
											  (257, 2, 128, (F32, 48)), (1000, 257, 10, (BF16, 384)), (1000, 1000, 1, (BF16, 80)), (1, 1000, 128, (F32, 208))])
def test_query_and_list_counts_around_256(ops, gpu, nq, nlist, k, route):
	"""The layout / scatter kernels work per 256 queries, the prefix kernels step by 256 lists.  Many lists of 1..3 vectors (and a few of 0);
	with one or two lists the probe row names the same list twice."""
	dtype, dp = route
	g = np.random.default_rng(nq * 1009 + nlist)
	sizes = g.integers(1, 4, nlist) if nlist > 2 else np.array([130, 67][:nlist])
	if nlist > 2: sizes[g.integers(0, nlist, nlist // 20)] = 0
	nprobe = 8 if nlist > 2 else 3
	probe = _random_probe(g, nq, nprobe, nlist, invalid=0.1 if nlist > 2 else 0.0)
	_check(ops, gpu, sizes, probe, dp, dtype, k, vr=1, seed=nq + nlist)


def test_tile128_persistent_workgroups_walk_several_tiles(ops, gpu):
	"""More 128 x 128 tiles than resident workgroups: 4 lists of 2048 vectors, 4096 queries on all four -> 4 x 32 x 16 = 2048 tiles, two workgroups
	per compute unit walk four or more each, so the three generations of row metadata rotate and the next tile's prefetch runs under every tile.
	(The older paths have no persistent kernel: not run at this size.)"""
	probe = np.tile(np.arange(4, dtype=np.int32), (4096, 1))
	probe[::2] = probe[::2, ::-1]
	_check(ops, gpu, [2048] * 4, probe, 128, BF16, k=10, vr=8, seed=21, old_paths=False)


@pytest.mark.parametrize("dp", [128, 512])
def test_tile128_fewer_tiles_than_workgroups_of_one_xcd_row(ops, gpu, dp):
	"""Fewer than eight tiles (three): most of the first eight workgroups have nothing to do, and each of the others has no next tile."""
	probe = np.array([[0, 1], [1, -1], [0, 0]], dtype=np.int32)
	_check(ops, gpu, [200, 5], probe, dp, BF16, k=10, vr=1, seed=22)


@pytest.mark.parametrize("route", THREE, ids=_route_id)
@pytest.mark.parametrize("k", [1, 128])
def test_probe_rows_with_holes_repeats_and_empty_lists(ops, gpu, route, k):
	"""-1 entries, ids >= nlist, the same list twice, rows with only empty lists, rows with nothing valid at all; k = 128 is above most row lengths."""
	dtype, dp = route
	sizes = [0, 40, 0, 129, 7]
	g = np.random.default_rng(31)
	probe = _random_probe(g, 64, 4, 5, invalid=0.4)
	probe[0] = [-1, -1, -1, -1]
	probe[1] = [0, 2, 0, 2]
	probe[2] = [5, 6, 1000000, -7]
	probe[3] = [3, 3, 3, 3]
	probe[4] = [4, -1, 4, 5]
	probe[5] = [1, 3, 4, 1]
	_check(ops, gpu, sizes, probe, dp, dtype, k, vr=1, seed=31)


@settings(max_examples=_N or 20, deadline=None, derandomize=not _FUZZ, database=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(route=st.sampled_from(ROUTES), nlist=st.sampled_from([1, 2, 3, 17, 100, 257, 300]), shape=st.sampled_from(["tiny", "edges", "skewed", "equal"]),
	   nq=st.integers(1, 700), nprobe=st.integers(1, 9), k=st.sampled_from([1, 10, 64, 128]), vr=st.sampled_from([1, 2, 8]), invalid=st.sampled_from([0.0, 0.2]),
	   padx=st.sampled_from([0, 8, 40]), padq=st.sampled_from([0, 8, 40]), seed=st.integers(0, 10 ** 6))
def test_grouped_search_random(ops, gpu, route, nlist, shape, nq, nprobe, k, vr, invalid, padx, padq, seed):
	dtype, dp = route
	g = np.random.default_rng(seed)
	if shape == "tiny": sizes = g.integers(0, 4, nlist)
	elif shape == "edges": sizes = g.choice([0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257], nlist)
	elif shape == "skewed": sizes = g.multinomial(min(6000, 40 * nlist), g.dirichlet(np.ones(nlist) * 0.3))
	else: sizes = np.full(nlist, int(g.integers(1, 200)))
	if sizes.sum() > 12000: sizes = sizes // 4
	if nprobe * int(max(sizes.max(), 1)) * nq > 6_000_000: nq = max(1, 6_000_000 // (nprobe * int(max(sizes.max(), 1))))   # (the slotted matrix of the older path)
	_check(ops, gpu, sizes, _random_probe(g, nq, nprobe, nlist, invalid), dp, dtype, k, vr=vr, padx=padx, padq=padq, seed=seed)


# ------------------------------------------------------------------ B. a different, smaller search on the same scratch
@pytest.mark.parametrize("route", THREE, ids=_route_id)
def test_smaller_search_after_a_larger_one_on_the_same_scratch(ops, gpu, route):
	"""A search, then a DIFFERENT one that needs a smaller packed matrix -- fewer queries, a shorter pitch, other probes -- on the same scratch with
	nothing poisoned in between: what the first left in the scratch (its scores, pair lists, descriptors) must not reach the second result."""
	dtype, dp = route
	g = np.random.default_rng(41)
	sizes = np.array([300, 0, 129, 64, 1, 500, 77, 128])
	n, nlist = int(sizes.sum()), len(sizes)
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	X = g.integers(-2, 3, (n, dp)).astype(np.int64)
	Xd = _padded(X, dp, dtype, gpu)
	off_d, ids_d = torch.from_numpy(off).to(gpu), torch.from_numpy(ids).to(gpu)

	def search(nq, nprobe, k, seed, lists):
		gq = np.random.default_rng(seed)
		Q = gq.integers(-2, 3, (nq, dp)).astype(np.int64)
		probe = gq.choice(lists, (nq, nprobe)).astype(np.int32)
		got = ops.ivf_search_grouped(Xd, off_d, ids_d, sizes, _padded(Q, dp, dtype, gpu), torch.from_numpy(probe).to(gpu), k)
		torch.cuda.synchronize()
		return got, _reference(X, Q, off, ids, probe, k, ("packed",))["packed"]

	_poison(ops)
	first, want = search(600, 6, 64, 1, np.arange(nlist))
	state = _scratch_state(ops)
	# (sizes_host is the same array: the pitch shrinks with nprobe, 6 -> 2; the second search stays on the short lists)
	second, want2 = search(70, 2, 100, 2, np.array([1, 2, 3, 4, 6, 7]))
	assert _scratch_state(ops) == state, "the second search was to reuse the first one's buffers"
	_equal(second, want2, "second (smaller) search")
	# (the first search ran on poison unless it had to grow the scratch; checked last so that a failure here does not mask the one above)
	_equal(first, want, "first search")


# ------------------------------------------------------------------ C. query chunking
@pytest.mark.parametrize("route", THREE, ids=_route_id)
@pytest.mark.parametrize("short_rows", [False, True])
def test_query_chunks(ops, gpu, route, short_rows):
	"""max_bytes = 1 puts both batched searches at their floor of 64 queries per chunk: 200 queries run as 64 + 64 + 64 + 8.  short_rows: lists of at
	most 3 vectors under k = 20 with nprobe = 2, so k_eff < k (6 in the packed search, 16 on the round-4 matrix with lmax = 8) pads inside the chunk loop.  Against the reference, then bit-equal to the
	unchunked call (in _check)."""
	dtype, dp = route
	g = np.random.default_rng(51 + short_rows)
	if short_rows:
		sizes, nprobe, k = g.integers(0, 4, 30), 2, 20
		sizes[0] = 3
	else:
		sizes, nprobe, k = g.integers(0, 150, 12), 4, 64
	_check(ops, gpu, sizes, _random_probe(g, 200, nprobe, len(sizes), invalid=0.1), dp, dtype, k, vr=2, seed=51, max_bytes=1)


# ------------------------------------------------------------------ D. the builder kernels
def _assignment(kind, n, nlist, g):
	if kind == "one": return np.full(n, nlist - 1)
	if kind == "round_robin": return np.arange(n) % nlist
	if kind == "sorted": return np.sort(g.integers(0, nlist, n))
	if kind == "reverse": return np.sort(g.integers(0, nlist, n))[::-1].copy()
	if kind == "random": return g.integers(0, nlist, n)
	a = g.integers(-3, nlist + 3, n)                              # "out_of_range": entries below 0 and at / past nlist among the valid ones
	if n: a[g.integers(0, n, 1 + n // 50)] = g.choice([-1, nlist, nlist + 5, 2 ** 31 - 1, -2 ** 31], 1 + n // 50)
	return a


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 1000, 100003])
def test_build_lists_equals_the_stable_counting_sort(ops, gpu, n):
	"""counts / offsets / ids against np.bincount, cumsum and a stable argsort, exactly.  The fill kernel cuts n into four 64-aligned quarters, the
	prefix kernel steps by 256 lists.  Entries outside [0, nlist) are dropped: offsets[-1] is the in-range count, ids is defined up to there."""
	g = np.random.default_rng(n)
	for nlist in (1, 2, 256, 257, 1000):
		for kind in ("one", "round_robin", "sorted", "reverse", "random", "out_of_range"):
			a = _assignment(kind, n, nlist, g).astype(np.int64)
			counts, offsets, ids = ops.ivf_build_lists(torch.from_numpy(a.astype(np.int32)).to(gpu), nlist)
			ok = (a >= 0) & (a < nlist)
			want_counts = np.bincount(a[ok], minlength=nlist)
			want_off = np.concatenate([[0], np.cumsum(want_counts)])
			keep = np.nonzero(ok)[0]
			want_ids = keep[np.argsort(a[keep], kind="stable")]
			what = f"n={n} nlist={nlist} {kind}"
			assert np.array_equal(counts.cpu().numpy(), want_counts), what
			assert np.array_equal(offsets.cpu().numpy(), want_off), what
			assert int(offsets[-1]) == int(ok.sum()), what
			assert ids.shape[0] == n and np.array_equal(ids.cpu().numpy()[:keep.size], want_ids), what


@pytest.mark.parametrize("d,padx,padc", [(1, 0, 0), (37, 3, 11), (256, 0, 8), (300, 20, 0)])
def test_list_means_on_integer_rows(ops, gpu, d, padx, padc):
	"""Integer-valued fp32 rows: every column sum is exact.  The kernel multiplies the exact sum by the rounded reciprocal of the count -- two roundings
	of 2^-24 each -- so a mean is within a relative 2^-22 of the fp64 quotient, and exact where the count is a power of two.  Empty lists keep
	their centroid bit for bit, and nothing is written past column d of a padded centroid row."""
	g = np.random.default_rng(d)
	sizes = np.array([0, 1, 2, 3, 0, 64, 100, 0, 7, 256, 1000, 1024, 5, 0])
	n, nlist = int(sizes.sum()), len(sizes)
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	X = g.integers(-8, 9, (n, d)).astype(np.int64)
	Xd = _padded(X, d + padx, torch.float32, gpu, fill=1000)
	before = torch.from_numpy(g.integers(-2 ** 31, 2 ** 31, (nlist, d + padc)).astype(np.int32))   # arbitrary bit patterns (NaNs among them)
	Cbuf = before.clone().view(torch.float32).to(gpu)
	out = ops.ivf_list_means(Xd, torch.from_numpy(off).to(gpu), Cbuf[:, :d])
	assert out.data_ptr() == Cbuf.data_ptr()
	after = Cbuf.cpu()
	assert torch.equal(after.view(torch.int32)[:, d:], before[:, d:]), "wrote into the padding of a centroid row"
	for l in range(nlist):
		if sizes[l] == 0:
			assert torch.equal(after[l].view(torch.int32), before[l]), f"empty list {l} lost its centroid"
			continue
		ref = X[off[l]:off[l + 1]].sum(axis=0).astype(np.float64) / float(sizes[l])
		got = after[l, :d].numpy().astype(np.float64)
		if sizes[l] & (sizes[l] - 1) == 0:
			assert np.array_equal(got, ref), f"list {l} of {sizes[l]} (a power of two): not exact"
		else:
			assert (np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref)).all(), f"list {l} of {sizes[l]}: {np.abs(got - ref).max()}"


def _norm_buckets(ops, M, n_buckets):
	from anncur_amd import _lib
	n = M.shape[0]
	norms = torch.empty(n, dtype=torch.float32, device=M.device)
	mm = torch.empty(2, dtype=torch.int32, device=M.device)
	bucket = torch.empty(n, dtype=torch.int32, device=M.device)
	_lib.check(_lib.load().anncur_norm_buckets(ops._p(M), n, M.shape[1], ops._ld(M), n_buckets, ops._p(norms), ops._p(mm), ops._p(bucket), ops._stream()), "norm_buckets")
	torch.cuda.synchronize()
	return norms.cpu().numpy(), bucket.cpu().numpy()


def _buckets_reference(norms, n_buckets):
	"""norm_bucket_kernel's formula in numpy fp32, from the exact min / max.  A NaN norm counts as 0 for the min / max (norm_minmax_kernel) and sits
	at the minimum (norm_bucket_kernel).  Every step is one IEEE fp32 operation on both sides (the kernel's division is the correctly rounded
	sequence, no fast-math), so the restatement is exact: no bucket-edge exclusion is needed."""
	f = np.float32
	nan = np.isnan(norms)
	seen = np.where(nan, f(0), norms).astype(f)
	lo, hi = f(seen.min()), f(seen.max())
	v = np.where(nan, lo, norms).astype(f)
	span = f(hi - lo)
	if not span > 0: return np.zeros(norms.shape[0], dtype=np.int64)
	pos = ((hi - v).astype(f) / span).astype(f) * f(n_buckets)
	assert pos.dtype == np.float32
	return np.clip(pos.astype(np.int64), 0, n_buckets - 1)


@pytest.mark.parametrize("n,d,pad", [(1, 1, 0), (3, 37, 3), (4097, 64, 0), (10007, 300, 4)])
@pytest.mark.parametrize("n_buckets", [1, 2, 100, 256])
def test_norm_buckets_and_descending_norm_order(ops, gpu, n, d, pad, n_buckets):
	"""Integer rows: the squared norms are exact (<= 64 * 300) and must equal the int64 sums; the buckets must equal the fp32 formula; the order
	must be the stable counting sort of the buckets -- a permutation of range(n), largest norms first (bucket 0 holds the largest norms, so the
	bucket index never decreases along it, i.e. the norm bucket never increases), ascending row id inside a bucket.  A zero row and a NaN row ride along."""
	g = np.random.default_rng(n + n_buckets)
	M = (g.integers(-8, 9, (n, d)) * (g.random((n, d)) < g.random((n, 1)))).astype(np.int64)   # a sparsity per row: norms spread from 0 to the maximum
	Md = _padded(M, d + pad, torch.float32, gpu, fill=1000)
	want_norms = (M * M).sum(axis=1).astype(np.float32)
	if n >= 3:
		Md[1] = 0
		Md[2, d // 2] = float("nan")
		want_norms[1], want_norms[2] = 0, np.nan
	norms, bucket = _norm_buckets(ops, Md, n_buckets)
	assert np.array_equal(norms, want_norms, equal_nan=True)
	want_bucket = _buckets_reference(want_norms, n_buckets)
	assert np.array_equal(bucket, want_bucket), f"{int((bucket != want_bucket).sum())} buckets differ"
	if n >= 3: assert bucket[2] == bucket[1] == want_bucket.max()               # the NaN row sits with the zero row, at the minimum
	order = ops.descending_norm_order(Md, n_buckets).cpu().numpy().astype(np.int64)
	assert np.array_equal(np.sort(order), np.arange(n)), "not a permutation"
	b = want_bucket[order]
	assert (np.diff(b) >= 0).all(), "a smaller-norm bucket in front of a larger-norm one"
	assert (np.diff(order)[np.diff(b) == 0] > 0).all(), "row ids not ascending inside a bucket"
	assert np.array_equal(order, np.argsort(want_bucket, kind="stable"))


def test_descending_norm_order_all_norms_equal(ops, gpu):
	"""All norms equal: span = 0, one bucket, the identity order (n not a multiple of 4)."""
	g = np.random.default_rng(3)
	M = g.permuted(np.tile(np.array([3, -3, 1, 0, 2], dtype=np.int64), (1023, 1)), axis=1)
	Md = _padded(M, 8, torch.float32, gpu)
	norms, bucket = _norm_buckets(ops, Md, 256)
	assert (norms == 23).all() and (bucket == 0).all()
	assert np.array_equal(ops.descending_norm_order(Md, 256).cpu().numpy(), np.arange(1023))


def test_map_ids_unpacked(ops, gpu):
	"""anncur_ivf_map_ids on hand-built columns of the [nq x nprobe * lmax] matrix: slot = col / lmax, position = col % lmax; a -inf value (the
	padding of a list, [size, lmax), as the pre-filled matrix yields it), a negative column and a probe of -1 give -1."""
	from anncur_amd import _lib
	sizes = np.array([3, 0, 5, 8, 1])
	lmax, nprobe, k = 8, 3, 6
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = np.random.default_rng(0).permutation(int(sizes.sum())).astype(np.int32) + 100
	probe = np.array([[0, 2, 3], [4, -1, 0], [3, 3, 2], [1, 4, 2]], dtype=np.int32)
	col = np.array([[0, 2, 8, 12, 16, 23], [0, 1, 8, 16, 18, -1], [7, 8, 15, 16, 20, 0], [0, 8, 16, 17, 20, 9]], dtype=np.int32)
	val = np.full(col.shape, 1.0, dtype=np.float32)
	val[0, 5] = 2.5
	val[1, 1] = -np.inf   # column 1 of query 1: list 4 has one vector, position 1 is its padding
	# (column 8 of query 1 lies in slot 1, a probe of -1: -1 whatever the value)
	val[3, 0] = -np.inf   # list 1 is empty: all padding
	val[3, 5] = -np.inf   # position 1 of list 4 again
	want = np.full(col.shape, -1, dtype=np.int32)
	for q in range(col.shape[0]):
		for j in range(k):
			c = int(col[q, j])
			if c < 0 or not val[q, j] > -np.inf: continue
			l = int(probe[q, c // lmax])
			if l < 0: continue
			assert c % lmax < sizes[l], "a finite score in a list's padding is outside the kernel's contract"
			want[q, j] = ids[off[l] + c % lmax]
	assert (want >= 0).sum() >= 18
	dev = lambda a: torch.from_numpy(a).to(gpu)
	c_d, v_d, p_d, o_d, i_d = dev(col), dev(val), dev(probe), dev(off), dev(ids)
	out = torch.full(col.shape, -7, dtype=torch.int32, device=gpu)
	_lib.check(_lib.load().anncur_ivf_map_ids(ops._p(c_d), ops._p(v_d), col.shape[0], k, lmax, ops._p(p_d), nprobe, ops._p(o_d), ops._p(i_d), ops._p(out), ops._stream()), "ivf_map_ids")
	torch.cuda.synchronize()
	assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("nlist", [1, 255, 256, 257, 1000])
def test_slotted_tile_start_prefix(ops, gpu, nlist):
	"""The single-workgroup prefix sum of ivf.hip (ivf_prefix256: 256 lists per step, the total at index nlist) called directly:
	anncur_ivf_group_scores_dev with max_tiles = 0 returns after its tile-start kernel, and tile_start[0 .. nlist] must equal numpy's exclusive
	cumulative sum of ceil(pairs_l / 64) * ceil(size_l / 64).  List sizes and pair counts at the tile edges; one list, one step less one, one
	step, one step plus one, four steps.  Integers only.
	(The packed search's pair_off / tile_start lie inside its workspace at offsets that only a restatement of ivf.hip's ivf_search_ws would
	give -- anncur_ivf_search_workspace_bytes returns the total alone -- so they are checked through the whole searches above, at 257 and
	1000 lists.)"""
	from anncur_amd import _lib
	g = np.random.default_rng(nlist)
	edge = np.array([0, 1, 63, 64, 65, 129], dtype=np.int64)
	sizes, pairs = g.choice(edge, nlist), g.choice(edge, nlist)
	sizes[-1], pairs[-1] = 129, 129                               # (the last list has tiles: the total differs from the last start)
	want = np.concatenate([[0], np.cumsum(-(-pairs // 64) * -(-sizes // 64))]).astype(np.int32)
	dev = lambda a: torch.from_numpy(np.concatenate([[0], np.cumsum(a)]).astype(np.int32)).to(gpu)
	off_d, poff_d = dev(sizes), dev(pairs)
	tile_start = torch.full((nlist + 1,), -7, dtype=torch.int32, device=gpu)
	x = torch.zeros(16, dtype=torch.float32, device=gpu)          # operands, pair ids and scores: required, not touched without tiles
	pid = torch.zeros(1, dtype=torch.int32, device=gpu)
	_lib.check(_lib.load().anncur_ivf_group_scores_dev(ops._p(x), _lib.F32, 16, 16, ops._p(off_d), nlist, ops._p(x), 16, 1,
													   ops._p(pid), ops._p(poff_d), ops._p(tile_start), 0, 8, ops._p(x), ops._stream()), "ivf_group_scores_dev")
	torch.cuda.synchronize()
	assert np.array_equal(tile_start.cpu().numpy(), want)
