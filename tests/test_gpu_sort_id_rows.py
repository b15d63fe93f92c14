"""ops.sort_id_rows (anncur_sort_id_rows) and ops.exclusion_from_sorted_rows: rows of (id, score) pairs sorted by id on the
device, holes last, and the per-query exclusion built from them without a host pass.  Scores are distinct integers, so every pair can be
traced: the result is bit-equal to a stable numpy argsort of the ids with holes last.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 63, 64, 65, 1000, 2048]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def rows_for(w, seed):
	"""Rows of distinct ids below 10 w + 5: sorted, reversed, random, then random rows with one hole, with min(w, 7) holes, and all holes."""
	rng = np.random.default_rng(seed)
	base = [np.sort(rng.choice(10 * w + 5, w, replace=False)) for _ in range(6)]
	rows = [base[0], base[1][::-1], rng.permutation(base[2]), rng.permutation(base[3]), rng.permutation(base[4]), base[5]]
	rows = np.stack(rows).astype(np.int32)
	rows[3, rng.integers(0, w)] = -1
	rows[4, rng.choice(w, min(w, 7), replace=False)] = -1
	rows[5, :] = -1
	if w > 1:
		rows[5, 0] = -7   # any negative id is a hole
	return rows


def reference(ids, scores):
	key = np.where(ids < 0, np.int64(1) << 40, ids.astype(np.int64))
	order = np.argsort(key, axis=1, kind="stable")
	return np.take_along_axis(ids, order, 1), np.take_along_axis(scores, order, 1), (ids >= 0).sum(1).astype(np.int32)


@pytest.mark.parametrize("w", WIDTHS)
def test_sort_id_rows_matches_numpy(ops, w):
	ids = rows_for(w, w)
	scores = np.random.default_rng(w + 1).permutation(ids.size).reshape(ids.shape).astype(np.float32)   # distinct integers
	want = reference(ids, scores)
	got = ops.sort_id_rows(torch.from_numpy(ids).cuda(), torch.from_numpy(scores).cuda())
	torch.cuda.synchronize()
	for g, x in zip(got, want):
		assert np.array_equal(g.cpu().numpy(), x)
	# rows inside a wider buffer (a pitch), sorted in place
	buf_i = torch.full((ids.shape[0], w + 3), 12345, dtype=torch.int32).cuda()
	buf_s = torch.full((ids.shape[0], w + 3), -1.0, dtype=torch.float32).cuda()
	buf_i[:, :w], buf_s[:, :w] = torch.from_numpy(ids).cuda(), torch.from_numpy(scores).cuda()
	vi, vs = buf_i[:, :w], buf_s[:, :w]
	_, _, counts = ops.sort_id_rows(vi, vs, out=(vi, vs))
	torch.cuda.synchronize()
	assert np.array_equal(buf_i[:, :w].cpu().numpy(), want[0]) and np.array_equal(buf_s[:, :w].cpu().numpy(), want[1])
	assert np.array_equal(counts.cpu().numpy(), want[2])
	assert (buf_i[:, w:] == 12345).all() and (buf_s[:, w:] == -1.0).all()


@pytest.mark.parametrize("w", [1, 65, 1000])
def test_exclusion_from_sorted_rows_equals_exclusion(ops, w):
	ids = rows_for(w, 100 + w)[:3]                       # the three full rows
	scores = np.zeros(ids.shape, dtype=np.float32)
	s_ids, _, counts = ops.sort_id_rows(torch.from_numpy(ids).cuda(), torch.from_numpy(scores).cuda())
	want = ops.exclusion(ids, 3, None, s_ids.device)
	for got in (ops.exclusion_from_sorted_rows(s_ids, counts), ops.exclusion_from_sorted_rows(s_ids)):
		assert got.e_max == want.e_max == w
		assert got.off.dtype == want.off.dtype and torch.equal(got.off, want.off)
		assert got.ids.dtype == want.ids.dtype and torch.equal(got.ids, want.ids)


def test_exclusion_from_sorted_rows_refuses_a_hole(ops):
	ids = rows_for(64, 3)[:4]                            # row 3 holds one hole
	s_ids, _, counts = ops.sort_id_rows(torch.from_numpy(ids).cuda(), torch.zeros(ids.shape, dtype=torch.float32).cuda())
	with pytest.raises(ValueError, match="hole"):
		ops.exclusion_from_sorted_rows(s_ids, counts)
	with pytest.raises(ValueError, match="hole"):
		ops.exclusion_from_sorted_rows(s_ids)
