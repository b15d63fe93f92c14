"""TEST INFRASTRUCTURE ONLY -- the two index classes of anncur_amd/nearest_nbr.py restated on the host, defined without the GPU.

FAISS is absent, so the classes' parity is unpinned; their only anchor is the algorithm their own docstrings state, composed of steps
whose arithmetic is fixed.  This module restates that composition in numpy so that train / add / search can be held BIT FOR BIT:

  * scores (assignment, probe, the flat index' fp32 route): ops.gemm's contract, the k-ordered fp32 fmaf chain -- chain_scores();
  * top-1 / top-nprobe / top-k: descending, ties to the smaller index (the exact scan);
  * list building: a stable counting sort -- build_lists_ref();
  * list means: sum * (1.0f / (float)count), the sum of integer rows being exact in any order -- list_means_ref();
  * renormalisation: renorm_rows_kernel's order of operations in np.float32 -- renorm_rows_ref();
  * empty lists: FAISS' split_clusters as the class docstring states it -- split_empty_ref();
  * the searches inside the probed lists: exact integer scores under the three tie rules of the three kernels -- lists_search_ref()
    (moved here from tests/test_gpu_ivf_exact.py, which imports it back).

Python 3.10 has no math.fma: an fmaf is float32(float64(a) * float64(b) + float64(acc)), which is the single rounding of the fmaf
only if the fp64 sum is exact.  The product of two fp32 numbers always is (48 bits); the sum is checked per step with TwoSum
(inexact_steps), and a case that fails raises InexactStep: the caller draws other data.  tests/test_cpu_ivf_index_reference.py holds
this module on its own (against np.longdouble, against fp64 normalisation, and through the k-means objective).  No tests in here."""
import numpy as np
import torch

F32 = np.float32
PAD_SCORE = np.float32(np.finfo(np.float32).min)    # FAISS' CMin<float>::neutral(): the score of a slot without a result
SPLIT_EPS = 1.0 / 1024                              # FAISS' EPS of split_clusters


class InexactStep(ArithmeticError):
	"""An fp64 step a * b + acc of a restated fmaf was rounded: the restatement does not cover this data."""


# ------------------------------------------------------------------ the fmaf chain
def inexact_steps(p, acc):
	"""Boolean array: where the fp64 sum p + acc is NOT exact (Knuth's TwoSum: the error term of the rounded sum, itself computed
	exactly, is non-zero).  p, acc float64.  A NaN or infinite operand counts as inexact."""
	s = p + acc
	bb = s - p
	err = (p - (s - bb)) + (acc - bb)
	return err != 0


def chain_scores(A, B, check=True):
	"""S[m, n] = the fp32 chain  acc = 0; for k ascending: acc = fmaf(A[m, k], B[k, n], acc)  for A [M x K], B [K x N]; float32 [M x N].
	One numpy expression per k, every step in fp64 and rounded to fp32 once.  check: InexactStep if any fp64 step was rounded."""
	Aw, Bw = np.asarray(A, dtype=F32).astype(np.float64), np.asarray(B, dtype=F32).astype(np.float64)
	M, K = Aw.shape
	acc = np.zeros((M, Bw.shape[1]), dtype=F32)
	for k in range(K):
		p, a = Aw[:, k:k + 1] * Bw[k:k + 1, :], acc.astype(np.float64)
		if check and inexact_steps(p, a).any():
			raise InexactStep(f"chain_scores: step k = {k} is not exact in fp64")
		acc = (p + a).astype(F32)
	return acc


def descending_order(S, k):
	"""Columns of the k largest entries of every row of S, descending, ties to the smaller column (no NaN in S)."""
	assert not np.isnan(S).any()
	return np.argsort(-S.astype(np.float64), axis=1, kind="stable")[:, :k]


# ------------------------------------------------------------------ renorm_rows_kernel
def renorm_rows_ref(M):
	"""Rows of M rescaled as renorm_rows_kernel does it, every operation in np.float32 in the kernel's order.  Returns a new array.
	  thread t of 256:  s = 0; for c = t, t + 256, ..: s = fmaf(v, v, s)       (a thread without a column at some step: s stays; restated as
	                                                                           a zero column, fmaf(0, 0, s) = s for every s >= +0 and NaN)
	  per wave of 64:   for d = 32, 16, .., 1: s = s + s[lane ^ d]              (the xor butterfly: every lane ends with the same sum)
	  tot = (p0 + p1) + (p2 + p3) over the four waves;  tot not > 0 (zero, NaN): the row stays as it is
	  inv = 1.0f / sqrtf(tot) (both correctly rounded);  row[c] = row[c] * inv."""
	M = np.array(M, dtype=F32, ndmin=2)
	r, d = M.shape
	steps = max(1, -(-d // 256))
	P = np.zeros((r, steps * 256), dtype=np.float64)
	P[:, :d] = M
	s = np.zeros((r, 256), dtype=F32)
	with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
		for j in range(steps):
			v = P[:, j * 256:(j + 1) * 256]
			p, a = v * v, s.astype(np.float64)        # the square of an fp32 number is exact in fp64
			if j > 0:                                 # (the first step adds to zero: exact)
				bad = inexact_steps(p, a) & np.isfinite(p + a)   # (an infinite or NaN sum is the same in fp32 and fp64)
				if bad.any():
					raise InexactStep(f"renorm_rows_ref: the fmaf step {j} is not exact in fp64")
			s = (p + a).astype(F32)
		w = s.reshape(r, 4, 64)
		lane = np.arange(64)
		for dd in (32, 16, 8, 4, 2, 1):
			w = w + w[:, :, lane ^ dd]
			assert w.dtype == F32
		part = w[:, :, 0]
		tot = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
		assert tot.dtype == F32
		inv = F32(1.0) / np.sqrt(tot)
		assert inv.dtype == F32
		out = M * inv[:, None]
	assert out.dtype == F32
	keep = ~(tot > 0)
	out[keep] = M[keep]
	return out


def same_bits(a, b):
	"""Elementwise: the same fp32 bit pattern, or NaN on both sides (the sign and payload of a NaN that an operation PRODUCES differ between
	hosts and the device; a NaN that is merely kept is compared through the unchanged row)."""
	a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
	return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def edge_rows(d=37):
	"""(M, want): six rows and what renorm_rows makes of them, written down by hand (only the ordinary last row goes through renorm_rows_ref).
	0 all zero: unchanged.  1 one NaN: tot is NaN, not > 0: unchanged.  2 every square underflows to zero (1e-30^2 is below the smallest
	denormal): tot = 0, unchanged.  3 every square overflows: tot = inf, inv = 0, every element becomes a zero of its own sign.  4 one inf:
	tot = inf, inv = 0, inf * 0 = NaN there and signed zeros elsewhere.  5 an ordinary row."""
	g = np.random.default_rng(d)
	sgn = np.where(g.random(d) < 0.5, -1.0, 1.0)
	sgn[:2] = (1.0, -1.0)
	M = np.zeros((6, d), dtype=F32)
	M[1] = g.integers(1, 9, d) * sgn; M[1, d // 2] = np.nan
	M[2] = 1e-30 * sgn
	M[3] = 3e20 * sgn
	M[4] = g.integers(1, 9, d) * sgn; M[4, d // 3] = np.inf
	M[5] = g.integers(1, 9, d) * sgn
	want = M.copy()
	want[3] = np.copysign(0.0, M[3])
	want[4] = np.copysign(0.0, M[4]); want[4, d // 3] = np.nan
	want[5] = renorm_rows_ref(M[5:6])[0]
	return M, want


# ------------------------------------------------------------------ lists
def build_lists_ref(assign, nlist):
	"""(counts [nlist], offsets [nlist + 1], ids [n]): the stable counting sort of the assignment -- list after list, ascending id inside one."""
	assign = np.asarray(assign, dtype=np.int64)
	assert ((assign >= 0) & (assign < nlist)).all()
	counts = np.bincount(assign, minlength=nlist).astype(np.int64)
	offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
	return counts, offsets, np.argsort(assign, kind="stable").astype(np.int64)


def list_means_ref(Xs, offsets, C):
	"""C with row l replaced by float32(sum of list l's rows) * (1.0f / (float)count); an empty list keeps its row.  Xs: list-ordered rows,
	INTEGER valued with count * max|x| < 2^24, so that the kernel's sequential fp32 sum is exact whatever its order (asserted)."""
	Xs = np.asarray(Xs, dtype=np.float64)
	assert (Xs == np.rint(Xs)).all()
	C = np.array(C, dtype=F32)
	for l in range(C.shape[0]):
		beg, end = int(offsets[l]), int(offsets[l + 1])
		if end == beg: continue
		assert (end - beg) * np.abs(Xs[beg:end]).max() < 1 << 24
		inv = F32(1.0) / F32(end - beg)
		C[l] = Xs[beg:end].sum(axis=0).astype(F32) * inv
	assert C.dtype == F32
	return C


def split_empty_ref(C, counts, rng, eps=SPLIT_EPS):
	"""FAISS' split_clusters: every empty list, in ascending order, takes over half of a heavy one.  The heavy list cj is drawn with weight
	max(count - 1, 0) (one rng.choice per empty list); list ci gets C[cj] * (1 + eps) on even columns and * (1 - eps) on odd ones, cj the
	mirror image (fp32 products, 1 +- 2^-10 being exact); ci takes half of cj's count, cj keeps the rest.  Returns the new C."""
	C = np.array(C, dtype=F32)
	nlist, d = C.shape
	counts = np.asarray(counts).astype(np.float64).copy()
	sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
	up, down = (1.0 + sign * eps).astype(F32), (1.0 - sign * eps).astype(F32)
	assert (up.astype(np.float64) == 1.0 + sign * eps).all() and (down.astype(np.float64) == 1.0 - sign * eps).all()
	for ci in np.flatnonzero(counts == 0):
		w = np.maximum(counts - 1.0, 0.0)
		cj = int(rng.choice(nlist, p=w / w.sum()))
		heavy = C[cj].copy()
		C[ci], C[cj] = heavy * up, heavy * down
		counts[ci] = counts[cj] / 2
		counts[cj] -= counts[ci]
	assert C.dtype == F32
	return C


def assign_ref(X, C):
	"""List of every row of X: the centroid of maximum chain score, ties to the smaller list."""
	return np.argmax(chain_scores(X, np.asarray(C).T), axis=1)    # (np.argmax returns the first maximum)


# ------------------------------------------------------------------ IVFFlatIPIndex
def train_ref(X, nlist, niter, seed=1234, max_points_per_centroid=256, spherical=True, renorm=renorm_rows_ref):
	"""The k-means of IVFFlatIPIndex.train on the host -> (centroids float32 [nlist x d], info).  One np.random.default_rng(seed) stream, drawn
	from in this order: the sub-sample (n > nlist * max_points_per_centroid: that many rows without replacement, kept in ASCENDING row order),
	one permutation whose first nlist entries are the initial centroids, then one choice per empty list per iteration.  The initial centroids
	are renormalised if spherical; an iteration is: assign, build lists, means (an empty list keeps its centroid), split, renormalise.
	info: "history" = the centroids after 0 .. niter iterations (what train with niter = t returns: the draws of iteration t come after those of
	the iterations before it), "empty" = the number of empty lists met in each iteration, "subsampled" = rows kept or None.
	renorm: the renormalisation (a test may pass the device's own, were its arithmetic not restatable)."""
	X = np.ascontiguousarray(X, dtype=F32)
	n = X.shape[0]
	assert n >= nlist
	rng = np.random.default_rng(seed)
	cap = nlist * max_points_per_centroid
	info = {"history": [], "empty": [], "subsampled": None}
	if n > cap:
		rows = np.sort(rng.choice(n, size=cap, replace=False))
		X, n, info["subsampled"] = X[rows], cap, rows
	C = X[rng.permutation(n)[:nlist]].copy()
	if spherical: C = renorm(C)
	info["history"].append(C.copy())
	for _ in range(niter):
		counts, offsets, ids = build_lists_ref(assign_ref(X, C), nlist)
		C = list_means_ref(X[ids], offsets, C)
		info["empty"].append(int((counts == 0).sum()))
		C = split_empty_ref(C, counts, rng)
		if spherical: C = renorm(C)
		info["history"].append(C.copy())
	return C, info


def add_ref(X, C):
	"""IVFFlatIPIndex.add on ALL vectors added so far -> (offsets [nlist + 1], ids [n], sizes [nlist], Xs [n x d]: the rows in list order)."""
	X = np.ascontiguousarray(X, dtype=F32)
	counts, offsets, ids = build_lists_ref(assign_ref(X, C), C.shape[0])
	return offsets, ids, counts, X[ids]


def probe_ref(Q, C, nprobe):
	"""[nq x min(max(nprobe, 1), nlist)]: every query's lists of largest chain score <q, c>, descending, ties to the smaller list."""
	nprobe = max(1, min(int(nprobe), C.shape[0]))
	return descending_order(chain_scores(Q, np.asarray(C).T), nprobe).astype(np.int32)


def lists_search_ref(X, Q, off, ids, probe, k, ties, lmax=1):
	"""The search on the host.  X [n x d], Q [nq x d] integer arrays, off [nlist + 1], ids [n], probe [nq x nprobe].  Per query: walk the probe slots
	in order, skip ids outside [0, nlist), concatenate the surviving lists' rows (list order) into the packed row, exact integer scores, sort
	descending with the tie rule, take min(k, len), map through ids; (-inf, -1) past that.
	ties -> {rule: (values fp32 [nq x k], ids int32 [nq x k])} for each rule asked for:
	  "packed":  the smaller packed column (a stable descending sort of the packed row);
	  "slotted": the smaller column slot * lmax + position in the list (the [nq x nprobe * lmax] matrix of ivf_scan_grouped);
	  "id":      the smaller vector id (ivf_scan's selection key).
	The sort is a top-k over the int64 keys score * 2^32 - tiebreak: the keys of a row are distinct, so it IS the stable descending sort.
	The products run in fp64 (every partial sum is an integer below 2^53: exact), then are taken as int64."""
	nq, nlist = Q.shape[0], len(off) - 1
	Xf, Qf = X.astype(np.float64), Q.astype(np.float64)
	out = {t: (np.full((nq, k), -np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int32)) for t in ties}
	for q0 in range(0, nq, 512):
		S = Qf[q0:q0 + 512] @ Xf.T
		for j in range(S.shape[0]):
			rows, cols = [], []
			for slot, l in enumerate(probe[q0 + j]):
				if 0 <= l < nlist:
					r = np.arange(off[l], off[l + 1], dtype=np.int64)
					rows.append(r)
					cols.append(slot * lmax + (r - off[l]))
			if not rows: continue
			rows = np.concatenate(rows)
			if rows.size == 0: continue
			s = S[j, rows].astype(np.int64)
			assert (s == S[j, rows]).all() and np.abs(s).max(initial=0) < 1 << 24
			m = min(k, rows.size)
			for t in ties:
				tb = np.arange(rows.size, dtype=np.int64) if t == "packed" else np.concatenate(cols) if t == "slotted" else ids[rows].astype(np.int64)
				assert t == "packed" or np.unique(tb).size == tb.size, "tie-break keys of one row must be distinct"
				order = torch.topk(torch.from_numpy(s * (1 << 32) - tb), m).indices.numpy()
				out[t][0][q0 + j, :m] = s[order]
				out[t][1][q0 + j, :m] = ids[rows[order]]
	return out


def exclusion_lists(exclude, nq):
	"""exclude= as the classes take it (one flat list for all queries, or one list per query) -> nq sets of ids."""
	if exclude is None:
		return [set()] * nq
	ex = list(exclude)
	if ex and isinstance(ex[0], (list, tuple, np.ndarray, range)):
		assert len(ex) == nq
		return [set(int(i) for i in r) for r in ex]
	return [set(int(i) for i in ex)] * nq


def filter_ref(vals, idx, excluded, k):
	"""The first k entries of every row that are neither holes (id < 0) nor excluded, in the row's order -> FAISS' convention:
	D float32 [nq x k], I int64 [nq x k], (-FLT_MAX, -1) in slots without a result."""
	nq = vals.shape[0]
	D, I = np.full((nq, k), PAD_SCORE, dtype=F32), np.full((nq, k), -1, dtype=np.int64)
	for q in range(nq):
		keep = [j for j in range(vals.shape[1]) if idx[q, j] >= 0 and int(idx[q, j]) not in excluded[q]][:k]
		D[q, :len(keep)], I[q, :len(keep)] = vals[q, keep], idx[q, keep]
	return D, I


def device_form(D, I):
	"""FAISS' (D, I) as search_device leaves the result on the device: int32 ids, -inf in slots without a result."""
	return np.where(I >= 0, D, F32(-np.inf)).astype(F32), I.astype(np.int32)


def search_ref(Xs, off, ids, C, Q, nprobe, k, ties, exclude=None):
	"""IVFFlatIPIndex.search on the host -> (D, I) in FAISS' convention.  Xs (list-ordered rows) and Q integer valued; off, ids from add_ref.
	Probe: probe_ref.  Inside the probed lists: lists_search_ref under the tie rule of the kernel that serves the call ("id": ivf_scan,
	"packed": the one-call grouped search, "slotted": ivf_scan_grouped, whose matrix gives every probe slot lmax = the longest list rounded
	up to 8 columns).  exclude: the search keeps k + the longest exclusion list candidates, then the first k allowed ones."""
	Xi, Qi = np.rint(np.asarray(Xs)).astype(np.int64), np.rint(np.asarray(Q)).astype(np.int64)
	assert (Xi == np.asarray(Xs)).all() and (Qi == np.asarray(Q)).all()
	excluded = exclusion_lists(exclude, Qi.shape[0])
	kc = k + max(len(e) for e in excluded)
	lmax = -(-max(int(np.diff(off).max()), 1) // 8) * 8
	vals, idx = lists_search_ref(Xi, Qi, np.asarray(off), np.asarray(ids), probe_ref(Q, C, nprobe), kc, (ties,), lmax)[ties]
	return filter_ref(vals, idx, excluded, k)


# ------------------------------------------------------------------ FlatIPIndex
def flat_search_ref(X, Q, k, exclude=None):
	"""FlatIPIndex.search (fp32) on the host -> (D, I) in FAISS' convention: the chain scores of every vector, descending, ties to the
	smaller id, excluded ids dropped, the first k."""
	S = chain_scores(Q, np.asarray(X, dtype=F32).T)
	order = descending_order(S, S.shape[1])
	return filter_ref(np.take_along_axis(S, order, axis=1), order, exclusion_lists(exclude, S.shape[0]), k)


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
NITER = 3
CASES = {   # integer data in [-8, 8]; n, d, nlist inside the ranges the exact tests are specified for
	"d24": dict(n=1500, d=24, nlist=7),                                    # d pads to 32 floats (fp32 lists) / 128 (bf16 lists); nlist odd
	"d64": dict(n=2048, d=64, nlist=16),                                   # no fp32 pad: the search takes the queries as they are
	"d130": dict(n=4096, d=130, nlist=64),                                 # d pads to 144 / 256; many short lists
	"prototypes": dict(n=1600, d=24, nlist=16, prototypes=8),              # 8 distinct vectors (a zero vector among them) x 200: at most 8 lists can be non-empty
	"subsample": dict(n=1500, d=64, nlist=16, max_points_per_centroid=8),  # 128 training rows of 1500
}
MAX_ATTEMPTS = 5
_DRAWN = {}


def case_data(name, attempt=0):
	"""The vectors of a case: float32 [n x d], integers in [-8, 8]; a pure function of (name, attempt)."""
	c = CASES[name]
	g = np.random.default_rng([sorted(CASES).index(name), attempt, 2026])
	if "prototypes" in c:
		protos = g.integers(-8, 9, (c["prototypes"], c["d"]))
		protos[3] = 0
		assert np.unique(protos, axis=0).shape[0] == c["prototypes"]
		return protos[g.permutation(np.arange(c["n"]) % c["prototypes"])].astype(F32)
	return g.integers(-8, 9, (c["n"], c["d"])).astype(F32)


def exact_case(name, spherical=True, niter=NITER):
	"""(X, centroids, info) of the first draw of the case on which every restated fmaf of train_ref and add_ref is exact (the TwoSum
	precondition); at most MAX_ATTEMPTS draws.  info["add"] = add_ref(X, centroids).  Computed once and shared: callers leave the arrays unchanged."""
	key = (name, spherical, niter)
	if key not in _DRAWN:
		c = CASES[name]
		for attempt in range(MAX_ATTEMPTS):
			X = case_data(name, attempt)
			try:
				C, info = train_ref(X, c["nlist"], niter, max_points_per_centroid=c.get("max_points_per_centroid", 256), spherical=spherical)
				info["add"] = add_ref(X, C)             # (the lists of ALL vectors under the final centroids: one more chain)
			except InexactStep:
				continue
			for a in [C] + info["history"] + list(info["add"]): a.setflags(write=False)   # (X stays writable: torch warns when it wraps a read-only array)
			_DRAWN[key] = (X, C, info)
			break
		else:
			raise AssertionError(f"case {name}: no draw in {MAX_ATTEMPTS} meets the exactness precondition")
	return _DRAWN[key]


def exact_queries(name, C, nq=40, seed=0):
	"""Integer queries in [-8, 8] on which the probe's chain is exact (redrawn like the cases)."""
	for attempt in range(MAX_ATTEMPTS):
		Q = np.random.default_rng([seed, attempt, 7]).integers(-8, 9, (nq, CASES[name]["d"])).astype(F32)
		try:
			chain_scores(Q, np.asarray(C).T)
		except InexactStep:
			continue
		return Q
	raise AssertionError(f"case {name}: no query draw in {MAX_ATTEMPTS} meets the exactness precondition")
