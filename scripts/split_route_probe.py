#!/usr/bin/env python
"""Times the three retrieval routes of a "rows" CUR index on one MI355X, in one process, alternating:

  fp32    ops.score_topk_dense            -- S_hat materialised in fp32 row chunks, then the exact scan
  bf16    ops.score_topk_fused            -- bf16 operands, S_hat never written, scores ~2e-3 from fp32
  bf16x3  ops.score_topk_split            -- split-bf16 operands on the fused kernel + fp32 rescore, fp32 values

Default shape: cfg2 size (10 000 queries x 100 000 items, fp32 A), 256 anchors, k = 100.  Two untimed warm-up calls per route, then
--reps rounds of one timed call per route (HIP events), the median printed as ms per call; for bf16x3 also the split into pack /
fused / rescore and the fraction of the bf16 matrix peak achieved, counted on 2 Q 3K I flop.  Then, for extra in {0, 16, 32, 64, 128}
candidates beyond k, the share of queries whose returned set differs from the dense route's (how SPLIT_RESCORE_EXTRA is chosen: the
smallest value at which the share stops falling).

    python scripts/split_route_probe.py [--queries 10000 --items 100000 --anchors 256 --k 100 --reps 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

import numpy as np
import torch

BF16_PEAK_TFLOPS = 2500.0   # MI355X dense bf16 matrix peak


def timed(fn):
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	out = fn()
	e1.record()
	e1.synchronize()
	return e0.elapsed_time(e1), out


def main(argv=None):
	ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
	ap.add_argument("--queries", type=int, default=10000)
	ap.add_argument("--items", type=int, default=100000)
	ap.add_argument("--anchors", type=int, default=256)
	ap.add_argument("--train", type=int, default=512)
	ap.add_argument("--k", type=int, default=100)
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--seed", type=int, default=0)
	args = ap.parse_args(argv)
	from anncur_amd import ops, synth
	from anncur_amd.cur import CURRowIndex
	dev = torch.device("cuda", 0)
	Q, I, K, k = args.queries, args.items, args.anchors, args.k
	A_train, A_test = synth.protocol_b(args.train, Q, I, dev, seed=args.seed, dtype=torch.float32)
	anc = np.sort(np.random.default_rng(args.seed).choice(I, K, replace=False))
	X = ops.gather_cols(A_test, anc)
	del A_test
	index = CURRowIndex(A_train, anc, compute_dtype="bf16x3")
	Et, sp = index._Et, index._split
	kp16 = ops.padded_k(K)
	from anncur_amd.cur import _norm_sorted_pack
	Etp16, ids16 = _norm_sorted_pack(Et, kp16)
	kc = ops.split_candidates(I, k)
	print(f"shape: Q={Q} I={I} K={K} k={k}  split Kp={sp.kp}  candidates kc={kc}  fused_supported={ops.fused_supported(Q, I, sp.kp, kc)}")

	routes = {
		"fp32": lambda: ops.score_topk_dense(X, Et, k),
		"bf16": lambda: ops.score_topk_fused(ops.pack_bf16(X, kp16), Etp16, I, k, leading_sample=True, item_ids=ids16),
		"bf16x3": lambda: ops.score_topk_split(X, Et, sp.sorted, I, k, item_ids=sp.item_ids, leading_sample=True),
	}
	for fn in routes.values():
		fn(); fn()
	torch.cuda.synchronize()
	ms = {name: [] for name in routes}
	parts = {"pack": [], "fused": [], "rescore": []}
	for _ in range(args.reps):
		for name, fn in routes.items():
			ms[name].append(timed(fn)[0])
		t, Xp = timed(lambda: ops.pack_split_bf16(X, 0, sp.kp)); parts["pack"].append(t)
		t, cand = timed(lambda: ops.score_topk_fused(Xp, sp.sorted, I, kc, leading_sample=True, item_ids=sp.item_ids)); parts["fused"].append(t)
		t, _ = timed(lambda: ops.rescore_topk(X, Et, cand.indices, k)); parts["rescore"].append(t)
	med = {n: statistics.median(v) for n, v in ms.items()}
	for n, v in ms.items():
		print(f"{n:7s} {med[n]:9.3f} ms per call   (min {min(v):.3f}, max {max(v):.3f}, {len(v)} calls)")
	pm = {n: statistics.median(v) for n, v in parts.items()}
	print(f"bf16x3 parts: pack {pm['pack']:.3f} ms, fused {pm['fused']:.3f} ms, rescore {pm['rescore']:.3f} ms")
	flop = 2.0 * Q * 3 * K * I
	print(f"bf16x3: 2 Q 3K I = {flop:.3e} flop -> {flop / (pm['fused'] * 1e-3) / 1e12:.1f} TFLOP/s in the fused call = "
		  f"{flop / (pm['fused'] * 1e-3) / 1e12 / BF16_PEAK_TFLOPS:.3f} of the bf16 peak ({flop / (med['bf16x3'] * 1e-3) / 1e12 / BF16_PEAK_TFLOPS:.3f} over the whole route)")
	print(f"bf16x3 / fp32 = {med['bf16x3'] / med['fp32']:.3f}   bf16x3 / bf16 = {med['bf16x3'] / med['bf16']:.3f}")

	want = np.sort(routes["fp32"]().indices.cpu().numpy(), 1)
	print("extra  kc    share of queries whose set differs from the dense route's")
	for extra in (0, 16, 32, 64, 128):
		got = ops.score_topk_split(X, Et, sp.sorted, I, k, item_ids=sp.item_ids, leading_sample=True, extra=extra)
		diff = (np.sort(got.indices.cpu().numpy(), 1) != want).any(1).mean()
		print(f"{extra:5d} {ops.split_candidates(I, k, extra):5d}  {diff:.5f}")
	b = np.sort(routes["bf16"]().indices.cpu().numpy(), 1)
	print(f" bf16 route, for comparison: {(b != want).any(1).mean():.5f}")


if __name__ == "__main__":
	main()
