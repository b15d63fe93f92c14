"""Sparse inner-product route probe: SparseIPIndex.search against FlatIPIndex.search on the densified matrix -- the only thing the
parent commit can do with TF-IDF data -- and the scoring launch alone, in one process.

  python scripts/sparse_route_probe.py [--parent-lib PATH/libanncur_hip.so] [--reps 21] [--out profiles/sparse_route_probe.json]

Data: Zipf-like synthetic TF-IDF with a fixed seed.  Every vector draws its terms from p(rank r) ~ 1 / r with replacement and keeps the distinct
ones (items: 290 draws, about 200 distinct terms; queries: 75 draws, about 60), so the few most frequent terms are in nearly every item and
most terms in a handful; values are tf x idf of the draws.  n = 30 000 items x V = 30 000 terms (densified: 3.6 GB) with the dense
comparison, n = 100 000 sparse-only (densified it would be 12 GB).  Q in {1, 64, 10 000}, k = 64.
Every timed call is one HIP-event pair around ONE call with two untimed calls of the same route in front of it; median and minimum of
--reps calls.  Per (n, Q): search on both index classes (host arrays in, host arrays out, as the reference's callers use them), the
scoring launch alone through ops.sparse_score_rows (which also allocates S), the postings it visits per second -- the sum of the document
frequencies of every query's terms -- and the bytes of S it writes per second.
--parent-lib: the library of the parent commit; the dense search runs on it too (the dense code paths are the same in both)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anncur_amd import _lib, ops  # noqa: E402
from anncur_amd.nearest_nbr import FlatIPIndex, SparseIPIndex  # noqa: E402

V, K = 30_000, 64
QS = (1, 64, 10_000)


class CSR(object):
	format = "csr"

	def __init__(self, indptr, indices, data, shape):
		self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape

	def rows(self, lo, hi):
		a, b = self.indptr[lo], self.indptr[hi]
		return CSR(self.indptr[lo:hi + 1] - a, self.indices[a:b], self.data[a:b], (hi - lo, self.shape[1]))

	def dense(self):
		out = np.zeros(self.shape, dtype=np.float32)
		out[np.repeat(np.arange(self.shape[0]), np.diff(self.indptr)), self.indices] = self.data
		return out


def zipf_tfidf(rng, n, draws):
	cdf = np.cumsum(1.0 / np.arange(1, V + 1))
	cdf /= cdf[-1]
	terms = np.sort(np.searchsorted(cdf, rng.random((n, draws))).astype(np.int32).clip(max=V - 1), axis=1)
	first = np.ones((n, draws), dtype=bool)
	first[:, 1:] = terms[:, 1:] != terms[:, :-1]
	counts = first.sum(axis=1)
	indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
	indices = terms[first]
	pos = np.flatnonzero(first.reshape(-1))
	tf = np.diff(np.concatenate([pos, [n * draws]])).astype(np.float32)      # run lengths: every row starts a run
	idf = np.log((1.0 + np.arange(1, V + 1, dtype=np.float64))).astype(np.float32)                        # rarer (higher rank) terms weigh more
	return CSR(indptr, indices, (tf * idf[indices]).astype(np.float32), (n, V))


def _parent_handle(path):
	lib = ctypes.CDLL(path)
	for name, (res, args) in _lib.SIGNATURES.items():
		fn = getattr(lib, name, None)
		if fn is not None:
			fn.restype, fn.argtypes = res, args
	return lib


class _use_lib(object):
	def __init__(self, handle):
		self.handle = handle

	def __enter__(self):
		self.saved, _lib._lib = _lib.load(), self.handle

	def __exit__(self, *exc):
		_lib._lib = self.saved


def _timed(fn):
	fn(); fn()
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b)


def _stats(ms):
	return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "n": len(ms)}


def probe(n, with_dense, reps, parent, rng):
	items = zipf_tfidf(rng, n, 290)
	all_q = zipf_tfidf(rng, max(QS), 75)
	sp = SparseIPIndex(V)
	sp.add(items)
	post = sp._index()
	df = np.diff(post.term_ptr.cpu().numpy())
	flat = None
	if with_dense:
		flat = FlatIPIndex(V)
		flat.add(items.dense())
	rows = []
	for Q in QS:
		q = all_q.rows(0, Q)
		dq = q.dense() if with_dense else None
		qdev = ops.SparseCSR(*(torch.as_tensor(a).cuda() for a in (q.indptr, q.indices, q.data)), Q, V)
		t = {"sparse_search": [], "dense_search": [], "dense_search_parent_lib": [], "score_rows": []}
		for _ in range(reps):
			t["sparse_search"].append(_timed(lambda: sp.search(q, K)))
			t["score_rows"].append(_timed(lambda: ops.sparse_score_rows(qdev, post)))
			if flat is not None:
				t["dense_search"].append(_timed(lambda: flat.search(dq, K)))
				if parent is not None:
					with _use_lib(parent):
						t["dense_search_parent_lib"].append(_timed(lambda: flat.search(dq, K)))
		visited = int(df[q.indices].sum())
		row = {"n": n, "V": V, "Q": Q, "k": K, "item_nnz": int(items.indices.size), "terms_per_item": items.indices.size / n, "terms_per_query": q.indices.size / Q,
			   "postings_visited": visited, "s_bytes": Q * n * 4, "plan": ops.sparse_plan(Q, n)}
		for name, ms in t.items():
			if ms:
				row[name] = _stats(ms)
		sec = row["score_rows"]["median_ms"] * 1e-3
		row["postings_per_s"] = visited / sec
		row["s_bytes_per_s"] = row["s_bytes"] / sec
		if flat is not None:      # same ids on both routes where the scores have no ties at the cut (values differ in the last bits: another summation order)
			a, b = sp.search(q, K)[1], flat.search(dq, K)[1]
			row["ids_equal_to_dense_frac"] = float((a == b).mean())
		rows.append(row)
		print(json.dumps(row), flush=True)
	del flat, sp, post
	torch.cuda.empty_cache()
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--parent-lib", default=None)
	ap.add_argument("--reps", type=int, default=21)
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_route_probe.json"))
	ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from (default: HEAD of this checkout)")
	args = ap.parse_args()
	parent = _parent_handle(args.parent_lib) if args.parent_lib else None
	commit = args.parent_commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
	rng = np.random.default_rng(2024)
	rows = probe(30_000, True, args.reps, parent, rng) + probe(100_000, False, args.reps, parent, rng)
	out = {"device": torch.cuda.get_device_name(0), "commit_parent": commit, "parent_lib": bool(parent), "reps": args.reps, "rows": rows}
	os.makedirs(os.path.dirname(args.out), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(out, f, indent=1)
	print("wrote", args.out)


if __name__ == "__main__":
	main()
