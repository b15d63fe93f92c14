"""anncur_rerank_scored and anncur_gather_pairs (csrc/pool.hip) against plain Python loops, bit for bit.

rerank_scored selects and moves (score, id) pairs and writes (-inf, -1): nothing is computed, so every output word has one right value --
`sorted` on (-score, id) over the pool of a query.  Every buffer of a call is a view into its own arena filled with poison (NaN bit
patterns for scores, 0x7f7f7f7f -- a valid positive id -- for ids): the inputs' arenas must be unchanged in every byte after the call,
the outputs' arenas unchanged outside the [Q x k_out] views.  The pad columns between the row pitches hold NaN (shared scores) and random
valid ids beside a score that would win (per-query rows), so a read past a per-query row's end shows up as a surplus candidate.  The
call takes no workspace.  Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 96
POISON32 = 0x7f7f7f7f
NAN32 = 0x7fc00123
NAN16 = 0x7fc1
MAX_TOPK = 2048
E_INVALID = -1

QS = (1, 5, 33)
N_SH = (0, 1, 63, 64, 65, 200, 4095, 4097)
N_PQ = (0, 1, 10, 257, 2048)


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


class Arena:
	"""A [rows x cols] view with row pitch ld inside a poisoned flat buffer of 16- or 32-bit words (floats travel as bit patterns).
	The pad columns of the view (ld > cols) hold `pad` (an array of the padded shape) or the poison."""

	def __init__(self, rows, cols, ld=None, poison=POISON32, dtype=torch.int32):
		self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
		self.n = (rows - 1) * self.ld + cols if rows and cols else 0
		self.buf = torch.full((2 * GUARD + self.n,), poison, dtype=dtype, device="cuda")
		self.poison = poison
		self.before = self.buf.cpu().numpy().copy()

	def set(self, a, pad=None):
		host = self.buf.cpu().numpy()
		flat = host[GUARD:GUARD + self.n]
		for r in range(self.rows):
			flat[r * self.ld:r * self.ld + self.cols] = a[r].view(host.dtype)
			if pad is not None and r + 1 < self.rows:
				flat[r * self.ld + self.cols:(r + 1) * self.ld] = pad[r, :self.ld - self.cols].view(host.dtype)
		self.buf.copy_(torch.from_numpy(host))
		self.before = host.copy()
		return self

	@property
	def ptr(self):
		return ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

	def unchanged(self):
		return np.array_equal(self.buf.cpu().numpy(), self.before)

	def read(self):
		"""(the view's rows, True if every word outside the view still holds the poison)"""
		host = self.buf.cpu().numpy()
		flat = host[GUARD:GUARD + self.n]
		rows = np.stack([flat[r * self.ld:r * self.ld + self.cols] for r in range(self.rows)])
		mask = np.ones(host.shape[0], dtype=bool)
		for r in range(self.rows):
			mask[GUARD + r * self.ld:GUARD + r * self.ld + self.cols] = False
		return rows, bool((host[mask] == self.poison).all())


def _bf16_bits(a):
	"""float32 array whose values are exact in bf16 -> uint16 bit patterns (as int16 for the arena)."""
	u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
	nan = np.isnan(a)
	assert ((u & 0xffff) == 0)[~nan].all(), "the case's scores must be exact in bf16"
	return np.where(nan, NAN16, u >> 16).astype(np.uint16).view(np.int16)


def _ranking(sh_ids, sh_val, pq_idx, pq_val):
	"""The whole pool of every query in the documented order: a list of Q lists of (score, id)."""
	shared = set(int(i) for i in sh_ids)
	out = []
	for q in range(pq_idx.shape[0] if pq_idx is not None else sh_val.shape[0]):
		pool = []
		if sh_val is not None:
			pool += [(float(v), int(i)) for v, i in zip(sh_val[q], sh_ids) if not np.isnan(v)]
		if pq_idx is not None:
			pool += [(float(v), int(i)) for v, i in zip(pq_val[q], pq_idx[q]) if i >= 0 and int(i) not in shared and not np.isnan(v)]
		out.append(sorted(pool, key=lambda e: (-e[0], e[1])))
	return out


def _expected(ranking, k_out):
	Q = len(ranking)
	ov = np.full((Q, k_out), -np.inf, dtype=np.float32)
	oi = np.full((Q, k_out), -1, dtype=np.int32)
	for q, r in enumerate(ranking):
		top = r[:k_out]
		ov[q, :len(top)] = [e[0] for e in top]
		oi[q, :len(top)] = [e[1] for e in top]
	return ov.view(np.int32), oi


ROW_KINDS = ("plain", "pq_holes", "sparse", "plain")


@functools.lru_cache(maxsize=None)
def _case(Q, n_sh, n_pq, shift=0, mode="random"):
	"""(sh_ids [n_sh], sh_val [Q x n_sh] or None, pq_idx, pq_val [Q x n_pq] or None, ranking).  Integer-valued scores in [-120, 120] (exact
	in bf16, tie-heavy).  Planted in every row, where the sizes allow: per-query ids equal to the first, a middle and the last shared id
	with a HIGHER score than the shared one (a kernel that kept them would rank them first); holes at the head, middle and tail; NaN,
	-inf and +inf in both sources; a tie between the sources.  Row kinds by (q + shift) % 4: plain; per-query source all holes; sparse
	(all but a handful of entries NaN or holes: fewer than k_out valid entries).  mode "ascending": scores strictly ascending along the
	pool (consecutive bf16 bit patterns), "equal": one score everywhere -- both without NaN and duplicates, to stay what they are about."""
	rng = np.random.default_rng(100003 * Q + 101 * n_sh + n_pq + 7 * shift)
	universe = 4 * (n_sh + n_pq) + 64
	sh_ids = np.sort(rng.choice(universe, n_sh, replace=False)).astype(np.int32)
	if n_sh > 1: sh_ids[0] = 0                                                 # id 0 takes part (still strictly ascending)
	outside = np.setdiff1d(np.arange(universe), sh_ids)
	sh_val = pq_idx = pq_val = None
	if n_sh:
		sh_val = rng.integers(-120, 121, (Q, n_sh)).astype(np.float32)
	if n_pq:
		pq_val = rng.integers(-120, 121, (Q, n_pq)).astype(np.float32)
		pq_idx = np.stack([rng.permutation(outside)[:n_pq] for _ in range(Q)]).astype(np.int32)
	if mode == "ascending":
		if n_sh: sh_val = np.tile(((0x3f80 + np.arange(n_sh, dtype=np.uint32)) << 16).view(np.float32), (Q, 1))
		if n_pq: pq_val = np.tile(((0x3f80 + n_sh + np.arange(n_pq, dtype=np.uint32)) << 16).view(np.float32), (Q, 1))
	elif mode == "equal":
		if n_sh: sh_val[:] = 3
		if n_pq: pq_val[:] = 3
	else:
		for q in range(Q):
			kind = ROW_KINDS[(q + shift) % 4]
			if n_sh >= 8:
				sh_val[q, rng.integers(n_sh, size=2)] = np.nan
				sh_val[q, rng.integers(n_sh)] = np.inf
				sh_val[q, rng.integers(n_sh)] = -np.inf
			if n_pq >= 10:
				free = list(rng.permutation(np.arange(1, n_pq - 1)))
				if n_sh:   # duplicates of shared ids: the shared score must stand
					for sid in sorted({int(sh_ids[0]), int(sh_ids[n_sh // 2]), int(sh_ids[-1])}):
						j = free.pop()
						pq_idx[q, j], pq_val[q, j] = sid, 1000 + j
					j = free.pop()   # a tie between the sources (ids differ: the smaller id wins)
					t = sh_val[q, n_sh // 3]
					pq_val[q, j] = 7 if np.isnan(t) else t
				pq_idx[q, 0], pq_idx[q, free.pop()], pq_idx[q, n_pq - 1] = -1, -1, -int(rng.integers(2, 1 << 30))   # holes: head, middle, tail
				pq_val[q, free.pop()] = np.nan
				pq_val[q, free.pop()] = np.inf
				pq_val[q, free.pop()] = -np.inf
			if kind == "pq_holes" and n_pq:
				pq_idx[q] = np.where(rng.random(n_pq) < 0.5, -1, -rng.integers(2, 1 << 30, n_pq))
			if kind == "sparse":
				if n_sh > 3: sh_val[q, rng.permutation(n_sh)[3:]] = np.nan
				if n_pq > 2: pq_idx[q, rng.permutation(n_pq)[2:]] = -1
	ranking = _ranking(sh_ids, sh_val, pq_idx, pq_val)
	return sh_ids, sh_val, pq_idx, pq_val, ranking


class Inputs:
	"""The input arenas of one case in one dtype / pitch variant; built once, checked unchanged after every call."""

	def __init__(self, case, bf16, pitched):
		sh_ids, sh_val, pq_idx, pq_val, _ = case
		self.n_sh, self.n_pq = sh_ids.size, 0 if pq_idx is None else pq_idx.shape[1]
		self.Q = sh_val.shape[0] if sh_val is not None else pq_idx.shape[0]
		self.dtype = 1 if bf16 else 0
		self.ld_sh = self.n_sh + (5 if pitched and self.n_sh else 0)
		self.ld_pq = self.n_pq + (3 if pitched and self.n_pq else 0)
		rng = np.random.default_rng(5)
		self.ids = self.sv = self.pi = self.pv = None
		if self.n_sh:
			self.ids = Arena(1, self.n_sh).set(sh_ids[None, :])
			if bf16:
				self.sv = Arena(self.Q, self.n_sh, self.ld_sh, poison=NAN16, dtype=torch.int16).set(_bf16_bits(sh_val))
			else:
				self.sv = Arena(self.Q, self.n_sh, self.ld_sh, poison=NAN32).set(sh_val)
		if self.n_pq:
			# the pad columns between the per-query rows hold random valid ids with a score that would rank first (the arena around the
			# views holds the NaN poison): a read past n_pq shows up as a surplus candidate
			self.pi = Arena(self.Q, self.n_pq, self.ld_pq).set(pq_idx, pad=rng.integers(0, 1 << 20, (self.Q, 8)).astype(np.int32))
			self.pv = Arena(self.Q, self.n_pq, self.ld_pq, poison=NAN32).set(pq_val, pad=np.full((self.Q, 8), 2000, dtype=np.float32))

	def call(self, lib, ops, k_out, expect=0, k_arg=None, **override):
		"""One launch with outputs [Q x k_out] in fresh poisoned arenas (k_arg: the k_out the library is told, where that is the bad argument)."""
		o_val, o_idx = Arena(self.Q, k_out, poison=NAN32), Arena(self.Q, k_out)
		ptr = lambda a: a.ptr if a is not None else None
		a = dict(sh_ids=ptr(self.ids), sh_val=ptr(self.sv), dtype=self.dtype, ld_sh=self.ld_sh, n_sh=self.n_sh, pq_idx=ptr(self.pi), pq_val=ptr(self.pv),
				 ld_pq=self.ld_pq, n_pq=self.n_pq, Q=self.Q, k_out=k_out if k_arg is None else k_arg, out_val=o_val.ptr, out_idx=o_idx.ptr)
		a.update(override)
		rc = lib.anncur_rerank_scored(a["sh_ids"], a["sh_val"], a["dtype"], a["ld_sh"], a["n_sh"], a["pq_idx"], a["pq_val"], a["ld_pq"], a["n_pq"], a["Q"],
									  a["k_out"], a["out_val"], a["out_idx"], ops._stream())
		assert rc == expect, (rc, lib.anncur_last_error())
		torch.cuda.synchronize()
		for arena in (self.ids, self.sv, self.pi, self.pv):
			assert arena is None or arena.unchanged(), "an input arena changed"
		if rc != 0:
			assert o_val.unchanged() and o_idx.unchanged(), "a refused call wrote to the outputs"
			return None
		gv, clean_v = o_val.read()
		gi, clean_i = o_idx.read()
		assert clean_v and clean_i, "written outside the [Q x k_out] outputs"
		return gv, gi


def _k_outs(n_sh, n_pq):
	"""Both sides of the edges of the three KMAX classes, clipped to the limits."""
	pool = n_sh + n_pq
	return sorted({min(k, pool, MAX_TOPK) for k in (1, 10, 128, 129, 512, 513, 2048, pool)})


def _check(got, ranking, k_out, what):
	want_v, want_i = _expected(ranking, k_out)
	gv, gi = got
	bad = np.nonzero((gi != want_i).any(1) | (gv != want_v).any(1))[0]
	assert bad.size == 0, f"{what}: {bad.size} queries differ, first q={bad[0]}\n got  {gi[bad[0]][:16]}\n want {want_i[bad[0]][:16]}\n got  {gv[bad[0]].view(np.float32)[:16]}\n want {want_v[bad[0]].view(np.float32)[:16]}"


@pytest.mark.parametrize("n_sh,n_pq", [(a, b) for a in N_SH for b in N_PQ if a + b])   # (an empty pool is an invalid argument: below)
def test_rerank_scored_bit_exact_in_poisoned_arenas(ops, n_sh, n_pq):
	"""The whole product of the shapes: every Q and k_out of one (n_sh, n_pq); fp32 and bf16 shared scores, contiguous and pitched rows."""
	from anncur_amd import _lib
	lib = _lib.load()
	for Q in QS:
		for shift in (range(4) if Q == 1 and n_sh + n_pq <= 400 else (0,)):
			case = _case(Q, n_sh, n_pq, shift)
			ranking = case[4]
			variants = [Inputs(case, bf16, pitched) for bf16, pitched in (((False, True), (True, False)) if n_sh else ((False, True), (False, False)))]
			for n, k_out in enumerate(_k_outs(n_sh, n_pq)):
				for v, inp in enumerate(variants):
					if Q == 33 and n_sh + n_pq > 4096 and (n + v) % 2:
						continue                                                      # the largest pools at Q = 33: each k_out in one of the two variants
					_check(inp.call(lib, ops, k_out), ranking, k_out, f"Q={Q} n_sh={n_sh} n_pq={n_pq} k_out={k_out} shift={shift} variant={v}")
			# the case holds what it is about
			if Q >= 5 and n_pq >= 10 and n_sh >= 8:
				k_all = min(n_sh + n_pq, MAX_TOPK)
				assert any(len(r) < k_all for r in ranking), "no row is short of k_out"
				assert any(e[0] == np.inf for e in ranking[0]) and any(e[0] == -np.inf for e in ranking[0])
				assert all(e[0] < 1000 or e[0] == np.inf for r in ranking for e in r), "a duplicate's per-query score was kept"


@pytest.mark.parametrize("mode", ["ascending", "equal"])
@pytest.mark.parametrize("n_sh,n_pq", [(4097, 2048), (200, 257), (0, 2048), (4097, 0)])
def test_worst_order_and_all_equal(ops, mode, n_sh, n_pq):
	"""Ascending scores: every offer beats the running threshold, the selector's worst order -- with 4097 + 2048 entries the pool crosses
	SEL_PASS, so a missing mid-stream compaction overflows the candidate buffer here.  All scores equal: the order is purely by id."""
	from anncur_amd import _lib
	lib = _lib.load()
	Q = 5
	case = _case(Q, n_sh, n_pq, 0, mode)
	ranking = case[4]
	assert all(len(r) == n_sh + n_pq for r in ranking)
	if mode == "equal":
		assert all([e[1] for e in r] == sorted(e[1] for e in r) for r in ranking)
	for bf16 in ((False, True) if n_sh else (False,)):
		inp = Inputs(case, bf16, pitched=not bf16)
		for k_out in _k_outs(n_sh, n_pq):
			_check(inp.call(lib, ops, k_out), ranking, k_out, f"{mode} n_sh={n_sh} n_pq={n_pq} k_out={k_out} bf16={bf16}")


def test_every_invalid_argument_is_refused_and_writes_nothing(ops):
	from anncur_amd import _lib
	lib = _lib.load()
	inp = Inputs(_case(5, 64, 10), bf16=False, pitched=True)
	for bad, msg in ((dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(Q=-1), "Q"), (dict(Q=1 << 31), "Q"),
					 (dict(n_sh=-1), "n_sh"), (dict(n_sh=65536, ld_sh=65536), "n_sh"), (dict(n_pq=-1), "n_pq"), (dict(n_pq=MAX_TOPK + 1, ld_pq=4096), "n_pq"),
					 (dict(n_sh=0, n_pq=0), "empty"), (dict(k_out=0), "k_out"), (dict(k_out=-3), "k_out"), (dict(k_out=75), "k_out"),
					 (dict(k_out=MAX_TOPK + 1), "k_out"), (dict(n_sh=0, k_out=11), "k_out"), (dict(n_pq=0, k_out=65), "k_out"),
					 (dict(ld_sh=63), "pitch"), (dict(ld_pq=9), "pitch"), (dict(sh_ids=None), "NULL"), (dict(sh_val=None), "NULL"),
					 (dict(pq_idx=None), "NULL"), (dict(pq_val=None), "NULL"), (dict(out_val=None), "null output"), (dict(out_idx=None), "null output")):
		k_out = bad.pop("k_out", 8)
		assert inp.call(lib, ops, max(k_out, 1), expect=E_INVALID, k_arg=k_out, **bad) is None
		assert msg in lib.anncur_last_error().decode(), (bad, lib.anncur_last_error())
	# the edges of the valid range
	case = _case(5, 64, 10)
	_check(inp.call(lib, ops, 74), case[4], 74, "k_out = pool")
	only_sh = _ranking(case[0], case[1], None, None)
	_check(inp.call(lib, ops, 64, n_pq=0, pq_idx=None, pq_val=None), only_sh, 64, "n_pq = 0 with NULL pointers")
	only_pq = _ranking(np.zeros(0, np.int32), None, case[2], case[3])
	_check(inp.call(lib, ops, 10, n_sh=0, sh_ids=None, sh_val=None), only_pq, 10, "n_sh = 0 with NULL pointers")
	assert lib.anncur_rerank_scored(None, None, 0, 0, 0, None, None, 0, 4, 0, 2, ctypes.c_void_p(8), ctypes.c_void_p(8), ops._stream()) == E_INVALID   # Q == 0 does not excuse NULL inputs
	o = torch.full((4,), 7, dtype=torch.int32, device="cuda")
	assert lib.anncur_rerank_scored(inp.ids.ptr, inp.sv.ptr, 0, inp.ld_sh, 64, inp.pi.ptr, inp.pv.ptr, inp.ld_pq, 10, 0, 2, ops._p(o), ops._p(o), ops._stream()) == 0
	torch.cuda.synchronize()
	assert (o == 7).all()                                                             # Q == 0: OK, nothing launched


def test_ops_rerank_scored_wrapper(ops):
	"""ops.rerank_scored: a TopK as `cand`, sliced (pitched) inputs, bf16 shared scores, a SharedIds built once, either source alone."""
	Q, n_sh, n_pq, k = 33, 65, 257, 40
	sh_ids, sh_val, pq_idx, pq_val, ranking = _case(Q, n_sh, n_pq)
	wide_i = torch.full((Q, n_pq + 3), 5, dtype=torch.int32, device="cuda")
	wide_v = torch.full((Q, n_pq + 3), float("nan"), device="cuda")
	wide_s = torch.full((Q, n_sh + 9), float("nan"), device="cuda")
	wide_i[:, :n_pq], wide_v[:, :n_pq], wide_s[:, :n_sh] = torch.from_numpy(pq_idx).cuda(), torch.from_numpy(pq_val).cuda(), torch.from_numpy(sh_val).cuda()
	shared = ops.shared_id_list(sh_ids, "cuda")
	assert shared.n == n_sh and shared.ids.dtype == torch.int32 and shared.ids.is_cuda
	cand = ops.TopK(wide_v[:, :n_pq], wide_i[:, :n_pq])
	for got in (ops.rerank_scored(k, cand, wide_v[:, :n_pq], sh_ids, wide_s[:, :n_sh]),
				ops.rerank_scored(k, wide_i[:, :n_pq].contiguous(), wide_v[:, :n_pq], shared, wide_s[:, :n_sh].bfloat16()),
				ops.rerank_scored(k, cand=wide_i[:, :n_pq], cand_scores=wide_v[:, :n_pq].contiguous(), shared_ids=list(map(int, sh_ids)), shared_scores=wide_s[:, :n_sh].contiguous())):
		assert got.values.dtype == torch.float32 and got.indices.dtype == torch.int32 and tuple(got.values.shape) == (Q, k)
		_check((got.values.cpu().numpy().view(np.int32), got.indices.cpu().numpy()), ranking, k, "ops.rerank_scored")
	got = ops.rerank_scored(k, shared_ids=shared, shared_scores=wide_s[:, :n_sh])
	_check((got.values.cpu().numpy().view(np.int32), got.indices.cpu().numpy()), _ranking(sh_ids, sh_val, None, None), k, "shared only")
	got = ops.rerank_scored(k, cand, wide_v[:, :n_pq])
	_check((got.values.cpu().numpy().view(np.int32), got.indices.cpu().numpy()), _ranking(sh_ids[:0], None, pq_idx, pq_val), k, "candidates only")
	with pytest.raises(ValueError, match="strictly ascending"):
		ops.rerank_scored(k, cand, wide_v[:, :n_pq], sh_ids[::-1].copy(), wide_s[:, :n_sh])
	with pytest.raises(ValueError, match=r"min\(322, 2048\) = 322"):
		ops.rerank_scored(323, cand, wide_v[:, :n_pq], shared, wide_s[:, :n_sh])


# ------------------------------------------------------------------ anncur_gather_pairs
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_gather_pairs_bit_exact(ops, n, bf16):
	"""A viewed inside a NaN buffer (lda > I), ids at 0, I - 1, -1 and I in every row, a pitched id list and a pitched output."""
	from anncur_amd import _lib
	lib = _lib.load()
	Q, I = 33, 301
	rng = np.random.default_rng(n)
	A = rng.integers(-120, 121, (Q, I)).astype(np.float32)
	idx = rng.integers(0, I, (Q, n)).astype(np.int32)
	for q in range(Q):
		for j, planted in zip(rng.permutation(n)[:4], rng.permutation([0, I - 1, -1, I])):
			idx[q, j] = planted
	if n == 1: idx[:4, 0] = [0, I - 1, -1, I]
	a_A = Arena(Q, I, I + 7, poison=NAN16, dtype=torch.int16).set(_bf16_bits(A)) if bf16 else Arena(Q, I, I + 7, poison=NAN32).set(A)
	a_idx = Arena(Q, n, n + 3).set(idx, pad=rng.integers(0, I, (Q, 8)).astype(np.int32))
	a_out = Arena(Q, n, n + 2, poison=NAN32)
	_lib.check(lib.anncur_gather_pairs(a_A.ptr, 1 if bf16 else 0, Q, I, I + 7, a_idx.ptr, n + 3, n, a_out.ptr, n + 2, ops._stream()), "gather_pairs")
	torch.cuda.synchronize()
	assert a_A.unchanged() and a_idx.unchanged()
	got, clean = a_out.read()
	assert clean, "written outside the [Q x n] output"
	valid = (idx >= 0) & (idx < I)
	want = np.take_along_axis(A, np.where(valid, idx, 0), axis=1)
	assert np.array_equal(got[valid], want.view(np.int32)[valid])
	assert np.isnan(got.view(np.float32)[~valid]).all() and (~valid).sum() >= 2
	# the wrapper, on a sliced matrix and a sliced id list
	Ad = torch.full((Q, I + 7), float("nan"), device="cuda")
	Ad[:, :I] = torch.from_numpy(A).cuda()
	if bf16: Ad = Ad.bfloat16()
	wide = torch.full((Q, n + 3), 0, dtype=torch.int32, device="cuda")
	wide[:, :n] = torch.from_numpy(idx).cuda()
	out = ops.gather_pairs(Ad[:, :I], wide[:, :n])
	assert out.dtype == torch.float32 and tuple(out.shape) == (Q, n)
	assert np.array_equal(out.cpu().numpy().view(np.int32)[valid], want.view(np.int32)[valid]) and torch.isnan(out.cpu())[torch.from_numpy(~valid)].all()


def test_gather_pairs_invalid_arguments(ops):
	from anncur_amd import _lib
	lib = _lib.load()
	A = torch.zeros((3, 8), device="cuda")
	idx = torch.zeros((3, 4), dtype=torch.int32, device="cuda")
	out = torch.full((3, 4), 7.0, device="cuda")
	p = ops._p
	good = dict(A=p(A), dtype=0, Q=3, I=8, lda=8, idx=p(idx), ld_idx=4, n=4, out=p(out), ldo=4)

	def rc(**kw):
		a = dict(good, **kw)
		return lib.anncur_gather_pairs(a["A"], a["dtype"], a["Q"], a["I"], a["lda"], a["idx"], a["ld_idx"], a["n"], a["out"], a["ldo"], ops._stream())

	for bad in (dict(dtype=2), dict(Q=-1), dict(I=0), dict(lda=7), dict(n=-1), dict(ld_idx=3), dict(ldo=3), dict(A=None), dict(idx=None), dict(out=None)):
		assert rc(**bad) == E_INVALID, bad
	torch.cuda.synchronize()
	assert (out == 7).all()
	assert rc(Q=0) == 0 and rc(n=0, A=None, idx=None, out=None) == 0 and rc() == 0
	torch.cuda.synchronize()
	assert (out == 0).all()
