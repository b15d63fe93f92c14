"""anncur_filter_topk (csrc/filter.hip) against a plain Python loop, bit for bit.

The kernel moves (score, id) pairs and writes (-inf, -1): nothing is computed, so every output word has one right value.  Every buffer
of a call -- scores, ids, segment offsets, segment ids, both outputs -- is a view into its own arena filled with poison (NaN bit
patterns / 0x7f7f7f7f, which as an id is a valid positive one): after the call the inputs' arenas must be unchanged in every byte, and
the outputs' arenas unchanged outside the [Q x k_out] views.  The pad columns of an input row (ld_in > n_cand) hold the same poison, so
a read past n_cand shows up as a surplus candidate.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNIVERSE = 6000          # item ids of the cases
GUARD = 96               # poisoned elements in front of and behind every view
POISON32 = 0x7f7f7f7f    # the poison of the id / offset arenas: as an int32 id a valid positive one
NAN32 = 0x7fc00123       # the poison of the score arenas: a NaN bit pattern


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


class Arena:
	"""A [rows x cols] view with row pitch ld inside a poisoned flat int32 / int64 buffer (floats travel as their bit patterns)."""

	def __init__(self, rows, cols, ld=None, poison=POISON32, dtype=torch.int32):
		self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
		self.n = (rows - 1) * self.ld + cols if rows else 0
		p = poison if dtype == torch.int32 else (poison << 32) | poison
		self.buf = torch.full((2 * GUARD + self.n,), p, dtype=dtype, device="cuda")
		self.poison = p

	def set(self, a):
		"""a: numpy [rows x cols] of the buffer's width (int32 / float32 / int64)."""
		host = self.buf.cpu().numpy()
		flat = host[GUARD:GUARD + self.n]
		for r in range(self.rows):
			flat[r * self.ld:r * self.ld + self.cols] = a[r].view(host.dtype)
		self.buf.copy_(torch.from_numpy(host))
		self.before = host.copy()
		return self

	@property
	def ptr(self):
		return ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

	def unchanged(self):
		return np.array_equal(self.buf.cpu().numpy(), self.before)

	def read(self):
		"""(the view's rows as numpy, True if every element outside the view still holds the poison)"""
		host = self.buf.cpu().numpy()
		flat = host[GUARD:GUARD + self.n]
		rows = np.stack([flat[r * self.ld:r * self.ld + self.cols] for r in range(self.rows)]) if self.rows else np.zeros((0, self.cols), host.dtype)
		mask = np.ones(host.shape[0], dtype=bool)
		for r in range(self.rows):
			mask[GUARD + r * self.ld:GUARD + r * self.ld + self.cols] = False
		return rows, bool((host[mask] == self.poison).all())


def _reference(val, idx, segs, k_out):
	"""The stable compaction in a loop: (float32 bit patterns as int32 [Q x k_out], ids int32 [Q x k_out])."""
	Q = val.shape[0]
	ov = np.full((Q, k_out), np.float32(-np.inf), dtype=np.float32)
	oi = np.full((Q, k_out), -1, dtype=np.int32)
	for q in range(Q):
		banned, p = set(int(x) for x in segs[q]), 0
		for v, i in zip(val[q], idx[q]):
			if p == k_out: break
			if i < 0 or int(i) in banned: continue
			ov[q, p], oi[q, p] = v, i
			p += 1
	return ov.view(np.int32), oi


def _call(lib, val, idx, ld_in, segs, k_out, shared=False):
	"""One launch with every buffer in a poisoned arena -> (values as int32 bits, ids); asserts that nothing outside the outputs changed.
	segs: Q ascending lists (shared: one list, given to the library without offsets)."""
	from anncur_amd import _lib, ops
	Q, n_cand = val.shape
	a_val = Arena(Q, n_cand, ld_in, poison=NAN32).set(val)
	a_idx = Arena(Q, n_cand, ld_in).set(idx)
	if shared:
		ids = np.asarray(segs, dtype=np.int32)
		a_off = None
	else:
		ids = np.concatenate([np.asarray(s, dtype=np.int32) for s in segs]) if Q else np.zeros(0, np.int32)
		off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
		a_off = Arena(1, Q + 1, dtype=torch.int64).set(off[None, :])
	a_ids = Arena(1, ids.size).set(ids[None, :]) if ids.size else None
	o_val, o_idx = Arena(Q, k_out, poison=NAN32), Arena(Q, k_out)
	_lib.check(lib.anncur_filter_topk(a_val.ptr, a_idx.ptr, ld_in, n_cand, Q, a_off.ptr if a_off else None, a_ids.ptr if a_ids else None,
									  ids.size if shared else 0, k_out, o_val.ptr, o_idx.ptr, ops._stream()), "filter_topk")
	torch.cuda.synchronize()
	for a in (a_val, a_idx, a_off, a_ids):
		assert a is None or a.unchanged(), "an input arena changed"
	gv, clean_v = o_val.read()
	gi, clean_i = o_idx.read()
	assert clean_v and clean_i, "written outside the [Q x k_out] outputs"
	return gv, gi


KINDS = ("empty", "first", "two", "all", "long", "random")


def _case(rng, Q, n_cand, shift):
	"""Rows and segments.  Segment kinds by (q + shift) % 6: empty; 1 id = the row's LEADING candidate; 2 ids = one of the row, one absent
	from it; 2048 ids that cover every candidate (all padding); 2048 ids whose first, middle and last element are candidates (the others
	mostly absent); a random list half drawn from the row.  Every row has holes (-1 and other negative ids) at random places."""
	val = np.zeros((Q, n_cand), dtype=np.float32)
	idx = np.zeros((Q, n_cand), dtype=np.int32)
	segs = []
	for q in range(Q):
		kind = KINDS[(q + shift) % 6]
		row = rng.permutation(UNIVERSE)[:n_cand].astype(np.int32)
		if kind == "empty":
			seg = []
		elif kind == "first":
			seg = [row[0]]
		elif kind == "two":
			absent = np.setdiff1d(np.arange(UNIVERSE), row)
			seg = [row[n_cand // 2], absent[rng.integers(absent.size)]]
		elif kind == "all":
			rest = np.setdiff1d(np.arange(UNIVERSE), row)
			seg = np.concatenate([row, rng.permutation(rest)[:2048 - n_cand]])
		elif kind == "long":
			seg = np.sort(rng.permutation(UNIVERSE)[:2048])
			plant = np.unique([seg[0], seg[1024], seg[-1]])[:n_cand]
			others = np.setdiff1d(row, plant)
			row = rng.permutation(np.concatenate([plant, others[:n_cand - plant.size]])).astype(np.int32)
		else:
			m = int(rng.integers(1, 100))
			seg = np.concatenate([row[rng.random(n_cand) < 0.5][:m], rng.integers(0, UNIVERSE, m)])
		seg = np.unique(np.asarray(seg, dtype=np.int64))
		assert row.size == n_cand and np.unique(row).size == n_cand
		holes = rng.random(n_cand) < 0.1
		if kind == "long": holes &= ~np.isin(row, plant)
		if kind != "first": row = np.where(holes, np.where(rng.random(n_cand) < 0.5, -1, -rng.integers(2, 1 << 30, n_cand)), row).astype(np.int32)
		idx[q] = row
		val[q] = -np.sort(-rng.integers(-50, 50, n_cand)).astype(np.float32) / 4      # descending, with ties
		segs.append(seg)
	return val, idx, segs


def _k_outs(n_cand):
	return sorted({1, n_cand, max(1, n_cand // 2 + 1)})


@pytest.mark.parametrize("Q", [1, 5, 67])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 129, 2048])
def test_filter_kernel_bit_exact_in_poisoned_arenas(ops, n_cand, Q):
	"""Row lengths around the 64-candidate chunk, k_out = 1 / middle / n_cand, Q = 1, 5 and 67 (four queries per workgroup: ragged last
	workgroups), contiguous rows and rows with a pitch, all six segment kinds at every Q."""
	from anncur_amd import _lib
	lib = _lib.load()
	rng = np.random.default_rng(1000 * n_cand + Q)
	for shift in (range(6) if Q == 1 else (0, 3) if Q == 5 else (0,)):
		val, idx, segs = _case(rng, Q, n_cand, shift)
		for k_out in _k_outs(n_cand):
			ld_in = n_cand + (0 if (k_out + shift) % 2 else 3)
			want_v, want_i = _reference(val, idx, segs, k_out)
			gv, gi = _call(lib, val, idx, ld_in, segs, k_out)
			what = f"n_cand={n_cand} Q={Q} k_out={k_out} ld_in={ld_in} shift={shift}"
			assert np.array_equal(gi, want_i), what
			assert np.array_equal(gv, want_v), what
			for q in range(Q):   # the cases do what they are about
				kind = KINDS[(q + shift) % 6]
				if kind == "all": assert (want_i[q] == -1).all()
				if kind == "first": assert want_i[q, 0] != idx[q, 0]
				if kind == "long" and n_cand >= 3: assert np.isin([segs[q][0], segs[q][1024], segs[q][-1]], idx[q]).all()


@pytest.mark.parametrize("n_cand,k_out", [(1, 1), (65, 40), (2048, 2048)])
@pytest.mark.parametrize("n_excl", [0, 1, 2, 2048])
def test_shared_set_equals_the_same_set_repeated_per_query(ops, n_cand, k_out, n_excl):
	from anncur_amd import _lib
	lib = _lib.load()
	rng = np.random.default_rng(n_cand + n_excl)
	Q = 9
	val, idx, _ = _case(rng, Q, n_cand, 0)
	seg = np.unique(np.concatenate([idx[rng.integers(Q), :n_excl // 2 + 1][:n_excl], rng.integers(0, UNIVERSE, 4 * n_excl)]))
	seg = seg[seg >= 0][:n_excl] if n_excl else seg[:0]
	if n_excl: assert seg.size == n_excl or n_excl == 2048
	want = _reference(val, idx, [seg] * Q, k_out)
	a = _call(lib, val, idx, n_cand + 5, seg, k_out, shared=True)
	b = _call(lib, val, idx, n_cand + 5, [seg] * Q, k_out)
	for got in (a, b):
		assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_ops_filter_topk_wrapper(ops):
	"""ops.filter_topk: raw lists through ops.exclusion (unsorted, duplicates), a sliced (pitched) input, int64 ids, an Exclusion."""
	rng = np.random.default_rng(5)
	Q, n_cand, k_out = 6, 130, 100
	val, idx, segs = _case(rng, Q, n_cand, 0)
	want_v, want_i = _reference(val, idx, segs, k_out)
	wide_v = torch.full((Q, n_cand + 7), float("nan"), device="cuda")
	wide_i = torch.full((Q, n_cand + 7), 3, dtype=torch.int32, device="cuda")
	wide_v[:, :n_cand], wide_i[:, :n_cand] = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
	messy = [list(rng.permutation(np.concatenate([s, s[:3]]))) for s in segs]
	for v, i, e in ((wide_v[:, :n_cand], wide_i[:, :n_cand], messy), (torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda().long(), messy),
					(wide_v[:, :n_cand], torch.from_numpy(idx).cuda(), ops.exclusion(segs, Q, UNIVERSE, "cuda"))):
		got = ops.filter_topk(v, i, e, k_out)
		assert got.values.dtype == torch.float32 and got.indices.dtype == torch.int32
		assert np.array_equal(got.indices.cpu().numpy(), want_i)
		assert np.array_equal(got.values.cpu().numpy().view(np.int32), want_v)
	none = ops.filter_topk(wide_v[:, :n_cand], wide_i[:, :n_cand], None, n_cand)   # holes only
	assert np.array_equal(none.indices.cpu().numpy(), _reference(val, idx, [[]] * Q, n_cand)[1])


def test_every_invalid_argument_is_refused(ops):
	from anncur_amd import _lib
	lib = _lib.load()
	Q, n = 3, 8
	v = torch.zeros((Q, n), device="cuda")
	i = torch.arange(Q * n, dtype=torch.int32, device="cuda").view(Q, n)
	ov = torch.full((Q, n), 7.0, device="cuda")
	oi = torch.full((Q, n), 7, dtype=torch.int32, device="cuda")
	off = torch.zeros(Q + 1, dtype=torch.int64, device="cuda")
	ids = torch.zeros(4, dtype=torch.int32, device="cuda")
	p = ops._p
	good = dict(in_val=p(v), in_idx=p(i), ld_in=n, n_cand=n, Q=Q, off=p(off), ids=p(ids), n_shared=0, k_out=4, out_val=p(ov), out_idx=p(oi))

	def rc(**kw):
		a = dict(good, **kw)
		return lib.anncur_filter_topk(a["in_val"], a["in_idx"], a["ld_in"], a["n_cand"], a["Q"], a["off"], a["ids"], a["n_shared"], a["k_out"], a["out_val"], a["out_idx"],
									  ops._stream())

	E = -1   # ANNCUR_E_INVALID
	for bad, msg in ((dict(k_out=0), "k_out"), (dict(k_out=n + 1), "k_out"), (dict(n_cand=0, k_out=0), "k_out"), (dict(n_cand=_lib.MAX_TOPK + 1, ld_in=4096), "n_cand"),
					 (dict(Q=0), "Q"), (dict(Q=-1), "Q"), (dict(ld_in=n - 1), "ld_in"), (dict(in_val=None), "null"), (dict(in_idx=None), "null"),
					 (dict(out_val=None), "null"), (dict(out_idx=None), "null"), (dict(off=None, n_shared=-1), "shared"),
					 (dict(off=None, ids=None, n_shared=2), "NULL"), (dict(out_val=p(v)), "alias"), (dict(out_idx=p(i)), "alias"),
					 (dict(out_idx=ctypes.c_void_p(i.data_ptr() + 4 * (Q * n - 1))), "alias"), (dict(out_idx=p(ov)), "alias")):
		assert rc(**bad) == E, bad
		assert msg in lib.anncur_last_error().decode(), (bad, lib.anncur_last_error())
	torch.cuda.synchronize()
	assert (ov == 7).all() and (oi == 7).all()                     # a refused call launches nothing
	# the edges of the valid range: accepted
	assert rc() == 0 and rc(off=None, ids=None, n_shared=0) == 0 and rc(ids=None) == 0 and rc(k_out=n) == 0 and rc(k_out=1) == 0
	torch.cuda.synchronize()
	assert np.array_equal(oi.cpu().numpy().ravel()[:Q], i.cpu().numpy()[:, 0])      # (the last call: k_out = 1, nothing excluded)
	with pytest.raises(_lib.AnncurHipError, match="k_out"):
		ops.filter_topk(v, i, None, n + 1)
