"""Probe of the sweep's A-fragment addresses (csrc/score16.hpp, Frag16Addr: NA base registers + immediates serve the K stagger steps).

Every (item row within a tile, k dimension) pair is individually visible in the result, so a wrong base or immediate for any lane or
step changes the answer:
  item i is one-hot at d_i = (161 (i // 32) + 5 (i % 32)) mod Kp with weight w_i = 1 + i mod 3 -- 161 is odd, so over any Kp
  consecutive tiles every row position meets every dimension;
  X[q, d] = 64 at d = (7 q + 3) mod Kp (7 is odd and Q > Kp: every dimension is some query's hot one), 1 + (q + d) mod 3 elsewhere.
All values are bf16-exact and all sums exact integers, so the result must be THE top-k (values descending, ties by ascending row) bit
for bit.  Query q's best are the items with d_i equal to its hot dimension, one per row position and round of Kp tiles, by weight and
then row; where k exceeds their number (Kp >= 128 at k = 100) the cold dimensions fill the rest.  A second check runs dense small
integers (|entries| <= 3) over the same shapes.

Shapes: Kp in {64, 128, 256}; Q = 300 = two row blocks, the second with 44 real queries (padded sub-tiles, and waves with no real
query); a whole number of rounds of Kp full tiles plus a partial tile of 17 items.  The fused path takes no fewer than 256 full tiles
(64 sampled tiles, each standing for at least four: plan_sample in csrc/score_fused.hip), so I = 32 max(Kp, 256) + 17: at Kp = 256 one
round, at Kp = 128 two, at Kp = 64 four -- the smallest I of that form the library accepts.  (At Kp = 64 a supported shape always
holds at least k items on a query's hot dimension -- full tiles >= max(256, 2 k), half an item per tile and dimension -- so there only
the dense check and the other queries' hot dimensions see a query's cold ones.)
The probe was run once against two builds with ONE wrong address each, both inside the tile image: step 9's immediate at Kp = 256
without its 256 bytes (the 3 cases of Kp = 256 fail), and step 2 on base register 0 (all 9 cases fail).
Needs an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
Q = 300
KPS = [64, 128, 256]


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _n_items(Kp):
	return 32 * max(Kp, 256) + 17


def _reference(S, k):
	"""THE top-k of integer scores S [Q x I] (int64, CPU): (values, rows), values descending, ties by ascending row."""
	I = S.shape[1]
	assert I < 1 << 27 and int(S.abs().max()) < 1 << 24
	key = S * (1 << 27) - torch.arange(I, dtype=torch.int64)   # one key per (score, row): larger score first, then smaller row
	rows = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows), rows


@functools.lru_cache(maxsize=None)
def _one_hot_case(Kp):
	"""(X [Q x Kp], E [Ip x Kp] zero-padded to whole tiles, S [Q x I] int64, d [I], hot [Q]) on the CPU; computed once per Kp, never written to."""
	I = _n_items(Kp)
	i = torch.arange(I, dtype=torch.int64)
	d = (161 * (i // 32) + 5 * (i % 32)) % Kp
	w = 1 + i % 3
	q = torch.arange(Q, dtype=torch.int64)
	hot = (7 * q + 3) % Kp
	X = 1 + (q[:, None] + torch.arange(Kp, dtype=torch.int64)[None, :]) % 3
	X[q, hot] = 64
	E = torch.zeros((-(-I // 32) * 32, Kp), dtype=torch.int64)
	E[i, d] = w
	S = X[:, d] * w[None, :]
	assert torch.equal(S, X @ E[:I].t())
	# over the full tiles every (row position, dimension) pair occurs, equally often
	pairs = torch.zeros((32, Kp), dtype=torch.int64)
	n_full = I // 32 * 32
	pairs.index_put_(((i % 32)[:n_full], d[:n_full]), torch.ones(n_full, dtype=torch.int64), accumulate=True)
	assert (pairs == max(Kp, 256) // Kp).all()
	assert hot.unique().numel() == Kp
	return X, E, S, d, hot


@functools.lru_cache(maxsize=None)
def _dense_case(Kp):
	I = _n_items(Kp)
	g = torch.Generator().manual_seed(9000 + Kp)
	X = torch.randint(-3, 4, (Q, Kp), generator=g)
	E = torch.zeros((-(-I // 32) * 32, Kp), dtype=torch.int64)
	E[:I] = torch.randint(-3, 4, (I, Kp), generator=g)
	return X, E, X @ E[:I].t()


def _run(ops, X, E, I, Kp, k):
	plan = ops.fused_plan(Q, I, Kp, k)
	assert plan["lg"] == 1 and plan["stage_pred"] == [2] and plan["n_tiles"] == max(Kp, 256) + 1, plan   # the 16x16x32 body, Kp-many rounds of tiles + a partial one
	Xp = X.to(torch.bfloat16).cuda()
	Etp = E.to(torch.bfloat16).cuda()
	assert torch.equal(Xp.cpu().long(), X) and torch.equal(Etp.cpu().long(), E)   # bf16-exact operands
	ws = ops.fused_workspace(Q, I, Kp, k, Xp.device)
	v, i = ops.score_topk_fused(Xp, Etp, I, k, workspace=ws)
	torch.cuda.synchronize()
	return v.cpu(), i.cpu().long()


@pytest.mark.parametrize("k", [32, 100])
@pytest.mark.parametrize("Kp", KPS)
def test_one_hot_items_make_every_row_and_dimension_visible(ops, Kp, k):
	X, E, S, d, hot = _one_hot_case(Kp)
	I = _n_items(Kp)
	v, i = _run(ops, X, E, I, Kp, k)
	want_v, want_rows = _reference(S, k)
	n_hot = (d[None, :] == hot[:, None]).sum(1)
	assert int(n_hot.min()) >= 32
	assert ((i >= 0) & (i < I)).all()
	bad = (v.double() != want_v.double()).any(1) | (i != want_rows).any(1)
	assert not bad.any(), f"Kp={Kp} k={k}: {int(bad.sum())} queries differ, first {int(bad.nonzero()[0])}: got {i[bad][0][:8].tolist()} {v[bad][0][:8].tolist()}, want {want_rows[bad][0][:8].tolist()} {want_v[bad][0][:8].tolist()}"
	# the top 32 lie on the query's hot dimension, heaviest first, then by row
	top = i[:, :32]
	assert (d[top] == hot[:, None]).all()
	assert (v[:, :32] >= 64).all()
	if k > int(n_hot.max()):   # the larger k reaches the cold dimensions
		assert (d[i[:, -1]] != hot).all() and (v[:, -1] <= 9).all()
	else:
		assert Kp == 64 or k == 32


@pytest.mark.parametrize("Kp", KPS)
def test_dense_small_integers_bit_for_bit(ops, Kp):
	X, E, S = _dense_case(Kp)
	I, k = _n_items(Kp), 100
	v, i = _run(ops, X, E, I, Kp, k)
	want_v, want_rows = _reference(S, k)
	assert ((i >= 0) & (i < I)).all()
	assert torch.equal(v.double(), want_v.double())
	assert torch.equal(i, want_rows)          # ties by ascending row
	assert int((want_v[:, 1:] == want_v[:, :-1]).sum()) > Q   # the case does hold ties
