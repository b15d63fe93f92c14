"""Reference of anncur_overlap_counts: Python sets, one query row and one pair at a time.  Nothing here follows the kernels'
lanes, halves or strides -- it is the definition they are held to."""
import numpy as np


def _ids(row, k):
	"""The set a prefix stands for: ids below zero (the selectors' -1 pads, or anything else negative) belong to no set."""
	return {int(x) for x in row[:k] if int(x) >= 0}


def overlap_ref(a, b, pairs):
	"""common[p, q] = |set(a[q, :ka_p]) & set(b[q, :kb_p])| for pairs = [(ka, kb), ...] -> int32 [n_pairs, Q]."""
	a, b = np.asarray(a), np.asarray(b)
	assert a.ndim == 2 and b.ndim == 2 and a.shape[0] == b.shape[0]
	out = np.zeros((len(pairs), a.shape[0]), dtype=np.int32)
	for p, (ka, kb) in enumerate(pairs):
		assert 0 <= ka <= a.shape[1] and 0 <= kb <= b.shape[1], (ka, kb)
		for q in range(a.shape[0]):
			out[p, q] = len(_ids(a[q], ka) & _ids(b[q], kb))
	return out


def first_pos(b_row, x):
	"""First position of id x in b_row, len(b_row) where it does not occur (and for a negative x, which is no id)."""
	if int(x) >= 0:
		for t, y in enumerate(b_row):
			if int(y) == int(x):
				return t
	return len(b_row)
