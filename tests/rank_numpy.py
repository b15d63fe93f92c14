"""The rank contract of include/anncur_hip.h, restated in NumPy.

    rank[q, j] = #{ i != id : S[q, i] > a  or  (S[q, i] == a and i < id) },   a = S[q, id],  id = ids[q, j]

the position of item id in row q sorted by score descending, ties to the smaller id.  The compare is the float compare (-0.0 == +0.0); a
NaN score is never ahead of anything (both compares are false); a target whose own score is NaN gets -1, and so does a hole (id == -1);
duplicate ids each report that item's rank.

rank_ref evaluates that count for every item of a row at once: a stable argsort of the negated row lists the items by (score descending,
id ascending) with every NaN at the end, so an item's position in the list is the number of items ahead of it.  rank_brute is the
sentence itself as a double loop; tests/test_cpu_rank_reference.py holds the two together on tie-heavy rows with NaN, +-inf and signed
zeros."""
import numpy as np


def rank_ref(S, ids):
	"""S [Q x I] float (compared as given), ids int [Q x t] in [-1, I) -> int32 [Q x t]."""
	S, ids = np.asarray(S), np.asarray(ids)
	Q, I = S.shape
	assert ids.ndim == 2 and ids.shape[0] == Q and ids.min(initial=0) >= -1 and ids.max(initial=-1) < I
	out = np.full(ids.shape, -1, dtype=np.int32)
	pos = np.empty(I, dtype=np.int64)
	for q in range(Q):
		row = S[q]
		pos[np.argsort(-row, kind="stable")] = np.arange(I)     # NaN sorts last; -0.0 and 0.0 compare equal and keep their id order
		idq = ids[q].astype(np.int64)
		ok = idq >= 0
		ok[ok] = ~np.isnan(row[idq[ok]])
		out[q, ok] = pos[idq[ok]]
	return out


def rank_brute(S, ids):
	S, ids = np.asarray(S), np.asarray(ids)
	out = np.full(ids.shape, -1, dtype=np.int32)
	for q in range(S.shape[0]):
		for j in range(ids.shape[1]):
			t = int(ids[q, j])
			if t < 0 or S[q, t] != S[q, t]:
				continue
			n = 0
			for i in range(S.shape[1]):
				if i != t and (S[q, i] > S[q, t] or (S[q, i] == S[q, t] and i < t)):
					n += 1
			out[q, j] = n
	return out


def bf16_round(x):
	"""fp32 array -> the nearest bf16 value (ties to even), as fp32."""
	u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
	u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
	return u.astype(np.uint32).view(np.float32)
