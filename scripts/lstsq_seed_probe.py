#!/usr/bin/env python
"""Timings of the incremental per-query solve and of its shared-prefix seed for DESIGN 4.4d (a record, not a gate), by the method of that
section's tables: one process, HIP events, each timed call queued behind two untimed ones, median of 7 with the minimum in brackets, ms per
call.  cfg2's size: Q = 10 000 queries, kq = 500 anchor queries, kc = 256 anchor items, k_step = 50.

    python scripts/lstsq_seed_probe.py [--out FILE.json]

  * state.extend 0 -> 306, 306 -> 356, 356 -> 406 and 406 -> 456 on an unseeded ops.LstsqState, with the Gram / factor / matvec split of
    timings= (a second, synchronising series);
  * state.seed_shared alone, and the seeded extend 256 -> 306 (the state is seeded again, untimed, in front of every call: an extension
    leaves z behind, and the next call on that state would no longer take the seeded path);
  * ops.lstsq_rows at n = 306, 356, 406 and 456 on the same rows;
  * AdaptiveSearcher.search at n_rounds = 2 and 4 (k_step = 50: solves at n = 306, and at 306, 356, 406) with incremental off, on without the
    seed and on with it: MatrixScorer on a 10 000 x 100 000 bf16 matrix (rank 32 + 0.3 noise), 500 anchor queries, 256 anchors, k = 10.
Every repeated extension n_old -> n_new runs on ONE state whose .n is put back to n_old in front of each call: the call re-forms the rows
from 16 (n_old / 16) down and leaves the ones above as they are, so it does the same work every time.
A build without seed_shared (an earlier commit, for the columns beside) runs the other lines and says so.  Needs an MI355X."""
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


def timed(fn, setup=None):
	"""ms of fn(): REPS times (two untimed calls, then the timed one between two events) -> (median, minimum).  setup() runs, untimed, in front
	of every one of the three calls."""
	ms = []
	for _ in range(REPS):
		for _ in range(2):
			if setup:
				setup()
			fn()
		if setup:
			setup()
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
	ap.add_argument("--kc", type=int, default=256)
	ap.add_argument("--k_step", type=int, default=50)
	ap.add_argument("--no_search", action="store_true", help="skip the AdaptiveSearcher lines")
	args = ap.parse_args()
	assert torch.cuda.is_available(), "lstsq_seed_probe needs a GPU"
	from anncur_amd import ops
	from anncur_amd.cur import CURRowIndex
	from anncur_amd.search import AdaptiveSearcher, MatrixScorer
	Q, m, kq, kc, k_step = args.Q, args.m, args.kq, args.kc, args.k_step
	has_seed = hasattr(ops.LstsqState, "seed_shared")
	if not has_seed:
		print("this build has no LstsqState.seed_shared: the seeded lines are left out", flush=True)
	dev = torch.device("cuda:0")
	g = torch.Generator(device=dev).manual_seed(0)
	sizes = [kc + r * k_step for r in range(1, 5)]                   # 306, 356, 406, 456
	cap = sizes[-1]
	out = {"Q": Q, "m": m, "kq": kq, "kc": kc, "k_step": k_step, "reps": REPS, "seed_shared": has_seed}

	def report(name, fn, setup=None):
		med, lo = timed(fn, setup)
		out[name] = [round(med, 3), round(lo, 3)]
		print(f"{name}: {med:.3f} ({lo:.3f}) ms", flush=True)

	# ---- the solve alone: rows that begin with kc shared items, then distinct items of their own
	pool = 4096
	Rt = torch.randn((pool, kq), generator=g, device=dev)
	shared = torch.randperm(kc, generator=g, device=dev).to(torch.int32)
	own = (torch.rand((Q, pool - kc), generator=g, device=dev).argsort(dim=1)[:, :cap - kc] + kc).to(torch.int32)
	ids = torch.cat([shared.view(1, -1).expand(Q, -1), own], dim=1).contiguous()
	C = torch.randn((Q, cap), generator=g, device=dev)
	W = torch.empty((Q, kq), dtype=torch.float32, device=dev)
	status = torch.empty((Q,), dtype=torch.int32, device=dev)
	st = ops.LstsqState(Rt, Q, cap)

	def extend(n_old, n_new, timings=None):
		st.n = n_old
		st.extend(ids[:, :n_new], C[:, :n_new], out=(W, status), timings=timings)

	for n_old, n_new in zip([0] + sizes[:-1], sizes):
		name = f"extend {n_old}->{n_new}"
		report(name, lambda: extend(n_old, n_new))
		assert int(status.sum().item()) == 0, "a query failed: the timing would be of the early exit"
		split = []
		for _ in range(REPS):
			extend(n_old, n_new)
			extend(n_old, n_new)
			extend(n_old, n_new, timings=split)
		parts = [[statistics.median(t[i] for t in split), min(t[i] for t in split)] for i in range(3)]
		out[name + " gram/factor/matvec"] = [[round(x, 3) for x in p] for p in parts]
		print(f"{name}: Gram {parts[0][0]:.3f} ({parts[0][1]:.3f}), factor {parts[1][0]:.3f} ({parts[1][1]:.3f}), matvec {parts[2][0]:.3f} ({parts[2][1]:.3f}) ms",
			  flush=True)
	if has_seed:
		def seed():
			st.n = 0
			st.seed_shared(shared)
		report(f"seed_shared {kc}", seed)
		name = f"seeded extend {kc}->{sizes[0]}"
		report(name, lambda: st.extend(ids[:, :sizes[0]], C[:, :sizes[0]], out=(W, status)), setup=seed)
		assert int(status.sum().item()) == 0
		split = []
		for _ in range(REPS):
			for timings in (None, None, split):
				seed()
				st.extend(ids[:, :sizes[0]], C[:, :sizes[0]], out=(W, status), timings=timings)
		parts = [[statistics.median(t[i] for t in split), min(t[i] for t in split)] for i in range(3)]
		out[name + " gram/factor/matvec"] = [[round(x, 3) for x in p] for p in parts]
		print(f"{name}: Gram {parts[0][0]:.3f} ({parts[0][1]:.3f}), factor {parts[1][0]:.3f} ({parts[1][1]:.3f}), matvec {parts[2][0]:.3f} ({parts[2][1]:.3f}) ms",
			  flush=True)
		# the same bits as the unseeded state and as lstsq_rows, at this size too
		W_seeded = W.clone()
		extend(0, sizes[0])
		W_rows, _ = ops.lstsq_rows(Rt, ids[:, :sizes[0]], C[:, :sizes[0]])
		same = bool(torch.equal(W_seeded.view(torch.int32), W.view(torch.int32)) and torch.equal(W.view(torch.int32), W_rows.view(torch.int32)))
		out["seeded == unseeded == lstsq_rows (bits)"] = same
		print(f"seeded extend, unseeded extend and lstsq_rows at n = {sizes[0]}: {'the same bits' if same else 'DIFFERENT BITS'}", flush=True)
	del st
	torch.cuda.empty_cache()
	for n in sizes:
		report(f"lstsq_rows n={n}", lambda: ops.lstsq_rows(Rt, ids[:, :n], C[:, :n], out=(W, status)))
	del Rt, ids, C, own
	torch.cuda.empty_cache()

	# ---- the search, 4.4d's setting
	if not args.no_search:
		rank, noise, k = 32, 0.3, 10
		U, V = torch.randn((kq + Q, rank), generator=g, device=dev), torch.randn((rank, m), generator=g, device=dev)
		A = (U @ V / rank ** 0.5 + noise * torch.randn((kq + Q, m), generator=g, device=dev)).bfloat16()
		del U, V
		anc = np.sort(np.random.default_rng(1).choice(m, kc, replace=False))
		index = CURRowIndex(A[:kq].contiguous(), anc)
		At = A[kq:].contiguous()
		del A
		scorer, qids = MatrixScorer(At), torch.arange(Q, dtype=torch.int64)
		variants = [("incremental off", {}), ("incremental, unseeded", {"incremental": True, "seed_shared": False} if has_seed else {"incremental": True})]
		if has_seed:
			variants.append(("incremental, seeded", {"incremental": True, "seed_shared": True}))
		for n_rounds in (2, 4):
			for label, kw in variants:
				s = AdaptiveSearcher(index, scorer, **kw)
				report(f"AdaptiveSearcher n_rounds={n_rounds} {label}", lambda: s.search(qids, k, k_step, n_rounds))
				out[f"AdaptiveSearcher n_rounds={n_rounds} {label} n_fallback"] = s.search(qids, k, k_step, n_rounds).n_fallback
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(out, f, indent=1)


if __name__ == "__main__":
	main()
