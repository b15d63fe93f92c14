"""Host-side data and references for tests/test_gpu_fused_kp512_wide_exact.py (no tests here; tests/gumbel_numpy.py is the precedent).

Everything is small-integer data: every bf16 operand and every fp32 partial sum of a score is exact, so a score matrix S [Q x I] built here
on the host (integers, never read back from the device) is what the kernels must compute bit for bit.  The references below are written
from the kernels' own definitions:
  - the prepass' sample and group layout: score_prepass_kernel<KP, GROUP> in csrc/score32.hpp (32-item tiles, tile_of) and
    wide_kernel<0, GROUP> in csrc/score_wide.hpp (256-item block tiles, bt_of; a block tile is eight 32-item sub-tiles in the same layout);
  - the threshold the sweep runs with: the k-th largest group maximum, cut to its 16-bit key prefix by the coarse threshold kernel
    (kth_value_wave_kernel in csrc/topk.hip) while a query has at most 4096 group maxima, exact above."""
import numpy as np
import torch

CHUNK_ROWS = 256   # queries per pass of the chunked host references (bounds the temporaries at the three-stage shapes)


# ------------------------------------------------------------------ the sweep bodies and the smallest shapes that reach them
# body -> (Kp, logical K, flags, {k: (I, lg, QT, ladder, stage_pred)}); I = the smallest the plan takes for the body at that k, + 17.
# Kp <= 256: 32 max(Kp, 256) + 17 = 8209 at k = 100; k = 700 needs 1400 full tiles (found with ops.fused_supported): 44817.
# qt1 is honoured from Kp = 128 on (at Kp = 64 the plan keeps QT = 2), and moves the shape to the 32x32x16 body; staged keeps the 16x16x32
# body up to k = 384 and takes 32x32x16 above.  Kp = 512: 8209; wide: 16 block tiles of 256 + 17 = 4113.
BODIES = {
	"ladder": (256, 250, {}, {100: (8209, 1, 2, True, 2), 700: (44817, 1, 2, True, 2)}),
	"staged": (64, 56, {"staged": True}, {100: (8209, 1, 2, False, 2), 700: (44817, 2, 2, False, 1)}),
	"mfma32": (128, 120, {"mfma32": True}, {100: (8209, 2, 2, False, 1), 700: (44817, 2, 2, False, 1)}),
	"qt1": (256, 200, {"qt1": True}, {100: (8209, 2, 1, False, 1), 700: (44817, 2, 1, False, 1)}),
	"q16": (512, 400, {}, {100: (8209, 1, 1, False, 4)}),
	"ring": (512, 257, {"mfma32": True}, {100: (8209, 2, 1, False, 1)}),
	"wide": (640, 513, {}, {100: (4113, 4, 2, False, 1)}),
}


# ------------------------------------------------------------------ operands
def dense_case(Q, I, K, seed, xmax=2, emax=2, const=False):
	"""X [Q x K] in [0, xmax], E [I x K] in [-emax, emax] (float32, integer-valued; const: E = 1), S = X E^T [Q x I] int32."""
	g = torch.Generator().manual_seed(seed)
	X = torch.randint(0, xmax + 1, (Q, K), generator=g).float()
	E = torch.ones(I, K) if const else torch.randint(-emax, emax + 1, (I, K), generator=g).float()
	assert max(xmax, 1) * max(emax, 1) * K < 1 << 24   # every partial sum is an exact integer in fp32, in any order
	return X, E, (X @ E.t()).to(torch.int32)


def sparse_x(Q, K, g, nnz=3, cmax=2):
	"""Each query: nnz coefficients from {1..cmax} at random columns over the whole [0, K) -> (X [Q x K] float32, col [Q x nnz], coef [Q x nnz] int8)."""
	col = torch.rand(Q, K, generator=g).topk(nnz, dim=1).indices   # (distinct columns per query)
	coef = torch.randint(1, cmax + 1, (Q, nnz), generator=g).to(torch.int8)
	X = torch.zeros(Q, K)
	X[torch.arange(Q)[:, None].expand(Q, nnz), col] = coef.float()
	return X, col, coef


def sparse_scores(E, col, coef):
	"""S[q] = sum_j coef[q, j] E[col[q, j]]: row gathers of E [K x I] int8 -> int8 [Q x I] (|S| <= 3 * 2 * 8 = 48)."""
	Q, I = col.shape[0], E.shape[1]
	S = torch.empty((Q, I), dtype=torch.int8)
	for q0 in range(0, Q, CHUNK_ROWS):
		sl = slice(q0, q0 + CHUNK_ROWS)
		acc = coef[sl, 0, None] * E[col[sl, 0]]
		for j in range(1, col.shape[1]):
			acc += coef[sl, j, None] * E[col[sl, j]]
		S[sl] = acc
	return S


def sparse_case(Q, I, K, seed, lo=-8, hi=8, nnz=3, cmax=2, plant=None):
	"""Sparse-X data: E [K x I] int8 in [lo, hi]; plant(E, g) may overwrite whole columns (items) before the scores are formed.
	Returns X [Q x K] float32, E [K x I] int8, S [Q x I] int8."""
	g = torch.Generator().manual_seed(seed)
	E = torch.randint(lo, hi + 1, (K, I), generator=g, dtype=torch.int8)
	if plant is not None:
		plant(E, g)
	X, col, coef = sparse_x(Q, K, g, nnz, cmax)
	assert nnz * cmax * max(abs(lo), abs(hi)) <= 127
	return X, E, sparse_scores(E, col, coef)


def device_operands(ops, X, E_items_by_k, Kp, ldx_pad=0):
	"""Packed device operands.  E_items_by_k: [I x K] (any dtype; a transposed view is fine).  ldx_pad > 0: query rows ldx_pad elements apart
	from packed, with poison (7.0) between the rows."""
	Xp = ops.pack_bf16(X.cuda(), Kp)
	if ldx_pad:
		wide = torch.full((X.shape[0], Kp + ldx_pad), 7.0, dtype=torch.bfloat16, device="cuda")
		wide[:, :Kp] = Xp
		Xp = wide[:, :Kp]
		assert Xp.stride(0) == Kp + ldx_pad or X.shape[0] == 1
	Etp = ops.pack_bf16(E_items_by_k.cuda().float(), Kp, row_multiple=32)
	I = E_items_by_k.shape[0]
	assert Etp.shape[0] == -(-I // 32) * 32 and not Etp[I:].any()
	return Xp, Etp


def poisoned_workspace(ops, Q, I, Kp, k):
	ws = ops.fused_workspace(Q, I, Kp, k, torch.device("cuda"))
	ws.fill_(0xff)
	return ws


# ------------------------------------------------------------------ references
def reference_topk(S, k):
	"""THE top-k of integer scores S [Q x I] (any integer dtype, CPU): (values int64, rows int64), values descending, ties by ascending row
	(one key per (score, row), as _reference in tests/test_gpu_fused_exact.py; in 32 bits where the key fits, by row chunks)."""
	Q, I = S.shape
	smax = int(S.abs().max())
	assert smax < 1 << 24
	shift = max(1, (I - 1).bit_length())
	kt = torch.int32 if (smax + 1) << shift < 1 << 31 else torch.int64
	ar = torch.arange(I, dtype=kt)
	rows = torch.empty((Q, k), dtype=torch.int64)
	for q0 in range(0, Q, CHUNK_ROWS):
		key = S[q0:q0 + CHUNK_ROWS].to(kt) * (1 << shift) - ar
		rows[q0:q0 + CHUNK_ROWS] = torch.topk(key, k, dim=1).indices
	return torch.gather(S, 1, rows).long(), rows


def count_ge(S, t):
	"""#{i : S[q, i] >= t[q]} per query (t: numpy [Q], values a float32 holds, as the scores are) -> int64 numpy [Q]."""
	Q = S.shape[0]
	out = np.empty(Q, dtype=np.int64)
	tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
	assert (tt.double().numpy() == np.asarray(t, dtype=np.float64)).all()
	for q0 in range(0, Q, CHUNK_ROWS):
		out[q0:q0 + CHUNK_ROWS] = (S[q0:q0 + CHUNK_ROWS].float() >= tt[q0:q0 + CHUNK_ROWS, None]).sum(1).numpy()
	return out


def coarse_floor(t):
	"""float32 numpy -> the value of its 16-bit sortable-key prefix with the low half zero (kth_value_wave_kernel, coarse): <= t, less than one
	bf16 ulp below.  Exact for integers of magnitude < 256 that are >= 0; a negative integer lands just below itself."""
	u = np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)
	s = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)) & np.uint32(0xffff0000)
	return np.where(s >> 31 != 0, s & np.uint32(0x7fffffff), ~s).astype(np.uint32).view(np.float32)


def sample_tiles(plan, I, leading, wide):
	"""The 32-item tiles the prepass samples, in the order of its group maxima."""
	n_st = plan["n_sample_tiles"]
	j = np.arange(n_st, dtype=np.int64)
	if not wide:
		return j if leading else (j * (I // 32)) // n_st                  # tile_of: over the FULL tiles
	bt = j if leading else (j * (I // 256)) // n_st                       # bt_of: over the full block tiles
	return (bt[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)


def group_rows(group):
	"""Rows of a 32-item tile per group maximum, in the order the prepass writes them: [groups per tile x items per group].
	C/D layout of the 32x32x16 MFMA: register e of lane half h holds item row (e & 3) + 8 (e >> 2) + 4 h."""
	if group == 16:   # gmax[2 j + h]: all sixteen registers
		return np.array([[(e & 3) + 8 * (e >> 2) + 4 * h for e in range(16)] for h in range(2)])
	return np.array([[(e & 3) + 8 * c + 4 * h for e in range(4)] for h in range(2) for c in range(4)])   # gmax[(2 j + h) 4 + c]: registers 4 c .. 4 c + 3


def reference_gmax(S, tiles, group):
	"""[Q x groups] float32: the group maxima of the sampled tiles from the host scores."""
	gr = torch.from_numpy(group_rows(group))
	items = (torch.from_numpy(tiles)[:, None, None] * 32 + gr[None, :, :])            # [tiles x groups per tile x items per group]
	assert int(items.max()) < S.shape[1]
	return S[:, items.reshape(-1)].view(S.shape[0], -1, gr.shape[1]).amax(dim=2).float()


def group_representatives(tiles, group):
	"""One item per sampled group (its first row), in the order of the group maxima."""
	return (tiles[:, None] * 32 + group_rows(group)[None, :, 0]).reshape(-1)


def bits(t):
	return t.contiguous().view(torch.int32)
