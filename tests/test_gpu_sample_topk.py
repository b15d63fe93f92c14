"""anncur_gumbel_noise and anncur_sample_topk (csrc/sample.hip) against the numpy statement of their contract
(tests/gumbel_numpy.py).

The noise: the 23-bit integer behind every known-answer point, invariance under row chunking and row position, accuracy of the two
logarithms against float64, and the distribution of a draw against the softmax / Plackett-Luce law.
The sampler: keys and ids bit for bit against a stable argsort of float32(float32(S * inv_T) + G) with the device's own G, at every size
around the vector, batch and selector boundaries, with S a view into a NaN-filled buffer of pitch I + 3 (every row alignment; a read
outside the row would drop an item) and the outputs pre-filled with 0xff.  Needs an MI355X."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_numpy as gn  # noqa: E402

pytestmark = pytest.mark.gpu

KNOWN = [   # (seed, stream, row_key, item) -> z >> 41 (the table of the header's contract; tests/test_cpu_sample_host.py checks the helper on it)
	((0, 0, 0, 0), 2363585),
	((1, 2, 3, 4), 5972515),
	((2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31 - 1), 5739042),
	((12345, 7, 100000, 99999), 5265390),
]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _bound(g64):
	"""|g_dev - g64| <= 2^-21 (1 + |g64|): with a 1-ulp logf the inner logarithm's relative error 2^-23 is an absolute 2^-23 in g, the outer
	logarithm and the rounding add 2^-23 |g|; the bound is that total times 4."""
	return 2.0 ** -21 * (1.0 + np.abs(g64))


# ------------------------------------------------------------------ the noise
@pytest.mark.parametrize("point, bits", KNOWN)
def test_noise_integer_level_at_the_known_answers(ops, point, bits):
	seed, stream, row_key, item = point
	assert int(gn.bits23(seed, stream, [row_key], [item])[0, 0]) == bits
	# item i is column i of a row of i + 1 items: the last point's row has 2^31 columns (8 GiB), of which a one-column view comes back
	g = ops.gumbel_noise(seed, stream, torch.tensor([row_key], dtype=torch.int64), item + 1)[:, item:]
	assert tuple(g.shape) == (1, 1)
	g_dev = float(g.cpu().numpy()[0, 0])
	del g
	torch.cuda.empty_cache()
	g64 = float(gn.gumbel64(seed, stream, [row_key], [item])[0, 0])
	err, bound = abs(g_dev - g64), float(_bound(g64))
	# the integer u 2^23 - 0.5 behind the device's g: d(u 2^23) / dg = 2^23 u (-ln u), so the bound on g is this many integers
	u = (bits + 0.5) * 2.0 ** -23
	tol = 2.0 ** 23 * u * -np.log(u) * bound * 1.01 + 1e-6
	got = float(gn.bits_from_gumbel(g_dev))
	print(f"{point}: g_dev = {g_dev!r}, g64 = {g64!r}, err / bound = {err / bound:.3f}, integer {got:.3f} against {bits} (tolerance {tol:.3f})")
	assert err <= bound
	assert abs(got - bits) <= tol and tol < 4


def test_noise_is_invariant_under_row_chunking_and_row_position(ops):
	Q, I = 37, 777
	rng = np.random.default_rng(5)
	keys = torch.from_numpy(rng.integers(0, 2 ** 32, Q, dtype=np.int64))
	whole = ops.gumbel_noise(9, 3, keys, I)
	parts = torch.cat([ops.gumbel_noise(9, 3, keys[:19], I), ops.gumbel_noise(9, 3, keys[19:], I)])
	assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
	perm = torch.from_numpy(rng.permutation(Q))
	assert torch.equal(ops.gumbel_noise(9, 3, keys[perm], I).view(torch.int32), whole[perm.cuda()].view(torch.int32))
	assert torch.equal(ops.gumbel_noise(9, 3, Q, I).view(torch.int32), ops.gumbel_noise(9, 3, torch.arange(Q), I).view(torch.int32))
	assert torch.equal(ops.gumbel_noise(9, 3, keys.cuda(), I).view(torch.int32), whole.view(torch.int32))            # keys already on the device
	assert not torch.equal(ops.gumbel_noise(9, 4, keys, I), whole) and not torch.equal(ops.gumbel_noise(10, 3, keys, I), whole)   # stream and seed count
	# more rows than one launch's grid.y: the rows beyond it come from the kernel's row loop
	tall = ops.gumbel_noise(9, 3, 70000, 3)
	assert torch.equal(tall[65530:65540].view(torch.int32), ops.gumbel_noise(9, 3, torch.arange(65530, 65540), 3).view(torch.int32))


def test_noise_accuracy_against_float64(ops):
	"""max |g_dev - g64| / (2^-21 (1 + |g64|)) over 64 x 16 384 draws; a maximum above 1 would mean a fast-math logarithm."""
	Q, I = 64, 16384
	keys = np.random.default_rng(6).integers(0, 2 ** 32, Q, dtype=np.int64)
	g_dev = ops.gumbel_noise(77, 5, torch.from_numpy(keys), I).cpu().numpy().astype(np.float64)
	g64 = gn.gumbel64(77, 5, keys, np.arange(I))
	err = np.abs(g_dev - g64)
	ratio = err / _bound(g64)
	print(f"noise accuracy over {Q} x {I}: max |g_dev - g64| = {err.max():.3e}, max err / bound = {ratio.max():.4f} (bound 2^-21 (1 + |g|)), "
		  f"g in [{g_dev.min():.3f}, {g_dev.max():.3f}]")
	assert np.isfinite(g_dev).all() and g_dev.min() >= -2.82 and g_dev.max() <= 16.64
	assert ratio.max() <= 1.0


def test_draw_follows_the_softmax_and_plackett_luce(ops):
	scores = np.array([0, 1, 2, 3, -1, 0.5], dtype=np.float32)
	Q = 20000
	S = torch.from_numpy(np.tile(scores, (Q, 1))).cuda()
	res = ops.sample_topk(S, 2, temperature=1.0, seed=0, stream=2)
	ids = res.indices.cpu().numpy()
	c1, c2 = gn.chi2_first_and_pairs(ids, scores)
	print(f"device draw: chi2 first item = {c1:.2f} (5 dof, 0.999 quantile 20.5), ordered pairs = {c2:.2f} (29 dof, 0.999 quantile 58.3)")
	assert c1 <= 20.5      # the 0.999 quantile at 5 degrees of freedom
	assert c2 <= 58.3      # the 0.999 quantile at 29 degrees of freedom


# ------------------------------------------------------------------ the sampler, bit for bit
def _pitched(S_host):
	"""S on the device as a view into a NaN-filled buffer: pitch I + 3, one guard row before and after."""
	Q, I = S_host.shape
	buf = torch.full((Q + 2, I + 3), float("nan"), dtype=torch.float32, device="cuda")
	view = buf[1:Q + 1, :I]
	view.copy_(torch.from_numpy(S_host))
	assert view.stride(0) == I + 3 or Q == 1
	return buf, view


def _raw_call(ops, view, k, inv_T, seed, stream, keys=None, off=None, ids=None, n_shared=0):
	"""anncur_sample_topk itself, outputs pre-filled with 0xff -> (keys as uint32, ids) on the host."""
	from anncur_amd import _lib
	Q, I = view.shape
	out_v = torch.full((Q, k), -1, dtype=torch.int32, device="cuda")
	out_i = torch.full((Q, k), -1, dtype=torch.int32, device="cuda")
	p = lambda t: ops._p(t) if t is not None else None
	rc = _lib.load().anncur_sample_topk(ops._p(view), view.stride(0) if Q > 1 else I + 3, Q, I, float(inv_T), seed, stream, p(keys), p(off), p(ids), n_shared, k,
										ops._p(out_v), ops._p(out_i), ops._stream())
	assert rc == 0, _lib.load().anncur_last_error()
	torch.cuda.synchronize()
	return out_v.cpu().numpy().view(np.uint32), out_i.cpu().numpy()


def _assert_same(got, want, what):
	(gv, gi), (wv, wi) = got, want
	assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5])
	assert np.array_equal(gv, wv.view(np.uint32)), (what, np.argwhere(gv != wv.view(np.uint32))[:5])


@pytest.mark.parametrize("I", [1, 2, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_sampler_bit_exact_around_every_boundary(ops, I):
	Q, seed, stream = 5, 11, 4
	inv_T = np.float32(1.0 / 0.7)
	rng = np.random.default_rng(I)
	S = (3.0 * rng.standard_normal((Q, I))).astype(np.float32)
	keys = rng.integers(0, 2 ** 32, Q, dtype=np.int64)
	buf, view = _pitched(S)
	G = ops.gumbel_noise(seed, stream, torch.from_numpy(keys), I).cpu().numpy()
	keys_dev = ops._row_keys(keys, Q, view.device, "test")
	for k in (1, 2, 128, 129, 512, 513, 2048):
		if k > I:
			continue
		_assert_same(_raw_call(ops, view, k, inv_T, seed, stream, keys_dev), gn.sample_reference(S, inv_T, G, k), (I, k))
	# row_keys = NULL: the row numbers
	G0 = ops.gumbel_noise(seed, stream, Q, I).cpu().numpy()
	_assert_same(_raw_call(ops, view, min(I, 7), inv_T, seed, stream), gn.sample_reference(S, inv_T, G0, min(I, 7)), (I, "row numbers"))
	assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isnan(buf[:, I:]).all()      # S is never written


def test_sampler_worst_order_for_the_selector(ops):
	"""S[q, i] = 1000 i at T = 1: the keys ascend whatever the noise, so every offer beats the running threshold and every batch compacts."""
	Q, I, k = 3, 4097 + 2048, 2048
	S = np.tile(1000.0 * np.arange(I, dtype=np.float32), (Q, 1))
	buf, view = _pitched(S)
	G = ops.gumbel_noise(1, 1, Q, I).cpu().numpy()
	want = gn.sample_reference(S, 1.0, G, k)
	assert np.array_equal(want[1], np.tile(np.arange(I - 1, I - 1 - k, -1, dtype=np.int32), (Q, 1)))      # (the premise)
	_assert_same(_raw_call(ops, view, k, 1.0, 1, 1), want, "ascending")


def test_small_temperature_is_the_exact_topk(ops):
	"""Distinct integer scores at T = 2^-6: gaps of 64 exceed the noise span of 19.5, so the drawn ids are rowwise_topk's."""
	Q, I, k = 4, 3000, 100
	rng = np.random.default_rng(3)
	S = np.stack([rng.permutation(I) for _ in range(Q)]).astype(np.float32)
	Sd = torch.from_numpy(S).cuda()
	got = ops.sample_topk(Sd, k, temperature=2.0 ** -6, seed=5, stream=1)
	assert torch.equal(got.indices, ops.rowwise_topk(Sd, k).indices)
	G = ops.gumbel_noise(5, 1, Q, I).cpu().numpy()
	_assert_same((got.values.cpu().numpy().view(np.uint32), got.indices.cpu().numpy()), gn.sample_reference(S, np.float32(64.0), G, k), "T = 2^-6")


def test_sampler_exclusion_nan_and_inf(ops):
	Q, I, k, seed, stream = 6, 300, 50, 21, 8
	rng = np.random.default_rng(9)
	S = rng.standard_normal((Q, I)).astype(np.float32)
	S[0, [3, 77, 299]] = np.nan
	S[1, [0, 150]] = -np.inf
	S[2, 10:40] = np.nan
	S[4, [5, 6]] = np.inf
	lens = [0, 1, 200, 0, 260, 1]                                   # row 4 keeps 40 < k allowed items: padded
	lists = [np.sort(rng.choice(I, n, replace=False)) for n in lens]
	Sd = torch.from_numpy(S).cuda()
	G = ops.gumbel_noise(seed, stream, Q, I).cpu().numpy()
	inv_T = np.float32(1.0 / 0.5)

	def run(exclude):
		r = ops.sample_topk(Sd, k, temperature=0.5, seed=seed, stream=stream, exclude=exclude)
		return r.values.cpu().numpy().view(np.uint32), r.indices.cpu().numpy()
	want = gn.sample_reference(S, inv_T, G, k, lists)
	assert (want[1][4, 40:] == -1).all() and (want[1][4, :40] >= 0).all() and np.isneginf(want[0][4, 40:]).all()      # (the premise: a padded row)
	assert not np.isin(want[1][0], [3, 77, 299]).any()                                                               # NaN is never drawn
	_assert_same(run([l.tolist() for l in lists]), want, "per-query lists")
	padded = np.full((Q, max(lens)), -1, dtype=np.int64)
	for q, l in enumerate(lists):
		padded[q, :l.size] = l[::-1]                                 # (any order: the host sorts)
	_assert_same(run(padded), want, "-1 padded array")
	_assert_same(run(ops.exclusion(padded, Q, I, Sd.device)), want, "an Exclusion passes through")
	shared = lists[2]
	_assert_same(run(shared), gn.sample_reference(S, inv_T, G, k, [shared] * Q), "one shared list")
	_assert_same(run(None), gn.sample_reference(S, inv_T, G, k), "no exclusion")
	# -inf is an ordinary candidate: with everything else excluded it is drawn, with key -inf and its id
	only = ops.sample_topk(Sd[1:2], 2, seed=seed, stream=stream, row_keys=[1], exclude=[i for i in range(I) if i not in (0, 150, 7)])
	assert only.indices.cpu().tolist() == [[7, 0]] and np.isneginf(only.values.cpu().numpy()[0, 1])


def test_key_ties_order_by_the_smaller_id(ops):
	Q, I, k = 4, 5000, 2048
	# the same row key twice: the same noise, so equal scores draw the same items
	S = torch.zeros((Q, I), dtype=torch.float32, device="cuda")
	r = ops.sample_topk(S, k, seed=2, stream=9, row_keys=[8, 3, 8, 2 ** 32 - 1])
	assert torch.equal(r.indices[0], r.indices[2]) and torch.equal(r.values[0].view(torch.int32), r.values[2].view(torch.int32))
	assert not torch.equal(r.indices[0], r.indices[1])
	# scores of 2^30 absorb the noise (an ulp of 128 against g < 16.64): every key of the row ties, and ties go to the smaller id
	big = torch.full((Q, I), 2.0 ** 30, dtype=torch.float32, device="cuda")
	r = ops.sample_topk(big, k, seed=2, stream=9)
	assert torch.equal(r.indices, torch.arange(k, dtype=torch.int32, device="cuda").expand(Q, k)) and bool((r.values == 2.0 ** 30).all())
	G = ops.gumbel_noise(2, 9, Q, I).cpu().numpy()
	_assert_same((r.values.cpu().numpy().view(np.uint32), r.indices.cpu().numpy()), gn.sample_reference(big.cpu().numpy(), 1.0, G, k), "all keys tie")


def test_sample_topk_dense_does_not_depend_on_the_chunking(ops):
	Q, I, K, k = 10, 1000, 24, 16
	rng = np.random.default_rng(12)
	X = torch.from_numpy(rng.standard_normal((Q, K)).astype(np.float32)).cuda()
	Et = torch.from_numpy(rng.standard_normal((I, K)).astype(np.float32)).cuda()
	keys = rng.integers(0, 2 ** 32, Q, dtype=np.int64)
	excl = [np.sort(rng.choice(I, n, replace=False)).tolist() for n in (0, 5, 1, 900, 0, 17, 3, 0, 64, 2)]
	kw = dict(temperature=0.8, seed=31, stream=6, row_keys=keys, exclude=excl)
	one = ops.sample_topk_dense(X, Et, k, **kw)
	three = ops.sample_topk_dense(X, Et, k, max_bytes=3 * 4 * I, **kw)                     # 3-row chunks: 3 + 3 + 3 + 1
	assert torch.equal(one.indices, three.indices) and torch.equal(one.values.view(torch.int32), three.values.view(torch.int32))
	direct = ops.sample_topk(ops.gemm(X, Et.t()), k, **kw)
	assert torch.equal(one.indices, direct.indices) and torch.equal(one.values.view(torch.int32), direct.values.view(torch.int32))
	# without row_keys the rows are named by their number in the CALL, not in the chunk
	a = ops.sample_topk_dense(X, Et, k, seed=31, stream=6)
	b = ops.sample_topk_dense(X, Et, k, seed=31, stream=6, max_bytes=3 * 4 * I)
	c = ops.sample_topk_dense(X, Et, k, seed=31, stream=6, row_keys=np.arange(Q))
	assert torch.equal(a.indices, b.indices) and torch.equal(a.indices, c.indices) and torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
	# ... and the host reference on the dense scores
	S = ops.gemm(X, Et.t()).cpu().numpy()
	G = ops.gumbel_noise(31, 6, torch.from_numpy(keys), I).cpu().numpy()
	_assert_same((one.values.cpu().numpy().view(np.uint32), one.indices.cpu().numpy()), gn.sample_reference(S, np.float32(1.0 / 0.8), G, k, excl), "dense")
