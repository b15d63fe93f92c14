#!/usr/bin/env python
"""Timings of the SoftMax item sampling for DESIGN 4.4e (a record, not a gate), by the method of the tables in 4.4c / 4.4d: one process, HIP
events, each timed call queued behind two untimed ones, median of 7 with the minimum in brackets, ms per call.  cfg2 size: Q = 10 000,
m = 100 000, kq = 500.

    python scripts/sample_probe.py [--out FILE.json]

  * ops.sample_topk (k = 50) beside ops.rowwise_topk (k = 50) on the same fp32 S: the exact scan reads the same bytes and is HBM-bound;
  * ops.sample_topk_dense (k = 50) on X [Q x 500], Et [m x 500];
  * AdaptiveSearcher.search at n_rounds = 2 and 4 with both strategies: MatrixScorer on a 10 000 x 100 000 bf16 matrix (rank 32 + 0.3 noise),
    500 anchor queries, 256 anchors, budget 256 + 200, k = 10 -- 4.4d's setting -- and recall@10 of each run on every 50th query.
Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

REPS = 7


def timed(fn):
	"""ms of fn(): REPS times (two untimed calls, then the timed one between two events) -> (median, minimum)."""
	ms = []
	for _ in range(REPS):
		fn()
		fn()
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		torch.cuda.synchronize()
		ms.append(a.elapsed_time(b))
	return statistics.median(ms), min(ms)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--out", default="")
	ap.add_argument("--Q", type=int, default=10000)
	ap.add_argument("--m", type=int, default=100000)
	ap.add_argument("--kq", type=int, default=500)
	args = ap.parse_args()
	assert torch.cuda.is_available(), "sample_probe needs a GPU"
	from anncur_amd import ops
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	Q, m, kq = args.Q, args.m, args.kq
	dev = torch.device("cuda:0")
	g = torch.Generator(device=dev).manual_seed(0)
	out = {"Q": Q, "m": m, "kq": kq, "reps": REPS}

	def report(name, fn):
		med, lo = timed(fn)
		out[name] = [round(med, 4), round(lo, 4)]
		print(f"{name}: {med:.3f} ({lo:.3f}) ms", flush=True)

	# the sampler beside the exact scan, on the same S
	X = torch.randn((Q, kq), generator=g, device=dev)
	Et = torch.randn((m, kq), generator=g, device=dev) / kq ** 0.5
	S = ops.gemm(X, Et.t())
	report("rowwise_topk k=50", lambda: ops.rowwise_topk(S, 50))
	report("sample_topk k=50 T=1", lambda: ops.sample_topk(S, 50, seed=1, stream=1))
	report("sample_topk k=50 T=0.05", lambda: ops.sample_topk(S, 50, temperature=0.05, seed=1, stream=1))
	del S
	report("sample_topk_dense k=50", lambda: ops.sample_topk_dense(X, Et, 50, seed=1, stream=1))
	report("score_topk_dense k=50", lambda: ops.score_topk_dense(X, Et, 50))
	del X, Et
	torch.cuda.empty_cache()

	# the adaptive search, 4.4d's setting
	rank, noise, n_anc, budget, k = 32, 0.3, 256, 200, 10
	U, V = torch.randn((kq + Q, rank), generator=g, device=dev), torch.randn((rank, m), generator=g, device=dev)
	A = (U @ V / rank ** 0.5 + noise * torch.randn((kq + Q, m), generator=g, device=dev)).bfloat16()
	del U, V
	anc = np.sort(np.random.default_rng(1).choice(m, n_anc, replace=False))
	index = CURRowIndex(A[:kq].contiguous(), anc)
	At = A[kq:].contiguous()
	del A
	scorer, qids = MatrixScorer(At), torch.arange(Q, dtype=torch.int64)
	some = torch.arange(0, Q, 50, device=dev)
	exact = ops.rowwise_topk(At[some].contiguous(), k).indices.cpu().numpy()
	for strategy in ("topk", "softmax"):
		for n_rounds in (2, 4):
			s = AdaptiveSearcher(index, scorer, strategy=strategy, temperature=1.0, seed=3)
			name = f"AdaptiveSearcher {strategy} n_rounds={n_rounds}"
			report(name, lambda: s.search(qids, k, budget // n_rounds, n_rounds))
			got = s.search(qids, k, budget // n_rounds, n_rounds).indices[some].cpu().numpy()
			rec = float(np.mean([np.isin(exact[q], got[q]).mean() for q in range(exact.shape[0])]))
			out[name + " recall@10"] = round(rec, 4)
			print(f"{name}: recall@{k} = {rec:.4f}", flush=True)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(out, f, indent=1)


if __name__ == "__main__":
	main()
