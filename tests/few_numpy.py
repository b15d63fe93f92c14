"""Launch 2 of the small-batch route (few_select_kernel, csrc/few.hip) restated in plain numpy.  A helper module, not a test:
tests/test_cpu_few_host.py holds it against topk_ref, tests/test_gpu_score_few_exact.py holds the kernel -- results AND the per-query
counters -- against it.

One score row [I] float32 ->
  group maxima     one per 64 consecutive items, NaN skipped, NaN for an all-NaN group (what launch 1 writes beside the scores);
  tau              the k-th largest non-NaN group maximum, -inf with fewer than k of them;
  collection       the maxima are walked in rounds of ROUND groups; a group with maximum >= tau is read and every v >= tau is a candidate;
  cap / fallback   more than cand_cap(k) candidates at the end of a round: the walk stops there and the row is scanned in full;
  result           the k best candidates (or of the row): score descending, smaller id on ties, NaN never, (-inf, -1) pads."""
import numpy as np

from topk_numpy import rerank_ref, topk_ref

GROUP = 64       # FEW_GROUP
ROUND = 1024     # FEW_ROUND
SEL_PASS = 4096  # select.hpp


def kmax_class(k):
	return 128 if k <= 128 else (512 if k <= 512 else 2048)


def cand_cap(k):
	"""The selector's buffer of the k class: SEL_PASS + 2 KMAX pairs."""
	return SEL_PASS + 2 * kmax_class(k)


def group_maxima(S):
	"""[Q x I] (or [I]) float32 -> [Q x ceil(I / 64)]: np.fmax skips a NaN next to a number, as the kernel's fmaxf chain from NaN does."""
	S = np.atleast_2d(np.asarray(S, dtype=np.float32))
	Q, I = S.shape
	G = -(-I // GROUP)
	P = np.full((Q, G * GROUP), np.nan, dtype=np.float32)
	P[:, :I] = S
	return np.fmax.reduce(P.reshape(Q, G, GROUP), axis=2)


def threshold(gm, k):
	real = gm[~np.isnan(gm)]
	if real.size < k:
		return np.float32(-np.inf)
	return np.float32(np.sort(real)[real.size - k])


def select_model(row, k):
	"""-> (values float32 [k], ids int32 [k], {"groups_read", "n_cand", "fallback", "tau"})."""
	x = np.asarray(row, dtype=np.float32).reshape(-1)
	gm = group_maxima(x)[0]
	tau = threshold(gm, k)
	cap = cand_cap(k)
	groups_read = n_cand = 0
	fallback = False
	cand = []
	with np.errstate(invalid="ignore"):
		for r0 in range(0, gm.size, ROUND):
			hit = np.flatnonzero(gm[r0:r0 + ROUND] >= tau) + r0
			groups_read += hit.size
			for g in hit:
				ids = np.arange(g * GROUP, min((g + 1) * GROUP, x.size))
				ids = ids[x[ids] >= tau]
				n_cand += ids.size
				cand.append(ids)
			if n_cand > cap:
				fallback = True
				break
	if fallback:
		val, ids = topk_ref(x, k)
	else:
		val, ids = rerank_ref(x, np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64), k)
	return val, ids, {"groups_read": groups_read, "n_cand": n_cand, "fallback": int(fallback), "tau": tau}
