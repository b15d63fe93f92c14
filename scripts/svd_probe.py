#!/usr/bin/env python
"""Times pinv.pinv_svd (Jacobi SVD + truncated pseudo-inverse) on anchor blocks of the synthetic protocol, beside the two
routes it could relieve: numpy.linalg.pinv on the host (fp32 values, as cur._pinv_host calls it) and pinv_newton_schulz_f64 where it
converges.  A record, not a gate: the table goes into DESIGN 4.5a and decides later whether "auto" should hand its ill-conditioned blocks
to this route.

One process.  Device figures: HIP events around the WHOLE call (decomposition, convergence reads, scaling, GEMM, rounding), each timed call
behind two untimed ones, the median of 7.  Host figures: wall clock, the median of 3.

usage: python scripts/svd_probe.py [--out FILE.json] [--blocks 512x256,512x512,...]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

import numpy as np
import torch

BLOCKS = "512x256,512x512,1024x1024,2048x1024"


def device_ms(fn, reps=7, untimed=2):
	out = []
	for _ in range(reps):
		for _ in range(untimed):
			fn()
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		b.synchronize()
		out.append(a.elapsed_time(b))
	return statistics.median(out)


def host_ms(fn, reps=3):
	out = []
	for _ in range(reps):
		t = time.perf_counter()
		fn()
		out.append((time.perf_counter() - t) * 1e3)
	return statistics.median(out)


def main(argv=None):
	ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
	ap.add_argument("--out", type=str, default="")
	ap.add_argument("--blocks", type=str, default=BLOCKS)
	ap.add_argument("--n_items", type=int, default=20000)
	args = ap.parse_args(argv)
	from anncur_amd import ops, pinv, synth
	dev = torch.device("cuda")
	rows_out = []
	for spec in args.blocks.split(","):
		rows, cols = (int(x) for x in spec.split("x"))
		A, _ = synth.protocol_b(rows, 1, args.n_items, dev, seed=0, rank=64, noise=0.05, dtype=torch.float32)
		anc = np.sort(np.random.default_rng(0).choice(args.n_items, cols, replace=False))
		W = ops.gather_cols(A, anc)
		X, info = pinv.pinv_svd(W, return_info=True)
		S = info["singular_values"].cpu().numpy()
		gE = (min(rows, cols) + 1) & ~1
		rec = {"block": spec, "cond_2": float(S[0] / S[-1]) if S[-1] > 0 else float("inf"), "sweeps": info["sweeps"], "converged": bool(info["converged"]),
			   "pair_launches": info["sweeps"] * (gE - 1), "svd_ms": device_ms(lambda: pinv.pinv_svd(W))}
		Wh = W.cpu().numpy()
		rec["numpy_host_ms"] = host_ms(lambda: np.linalg.pinv(Wh))
		Xh = np.linalg.pinv(Wh.astype(np.float64))
		rec["rel_err_vs_fp64"] = float(np.abs(X.cpu().numpy() - Xh).max() / np.abs(Xh).max())
		_, ns = pinv.pinv_newton_schulz_f64(W, return_info=True)
		rec["newton_schulz_converged"], rec["newton_schulz_iterations"] = bool(ns["converged"]), ns["iterations"]
		rec["newton_schulz_ms"] = device_ms(lambda: pinv.pinv_newton_schulz_f64(W)) if ns["converged"] else None
		rows_out.append(rec)
		print(json.dumps(rec), flush=True)
	print("| block | cond_2 | sweeps | pair launches | Jacobi SVD pinv (ms) | numpy host pinv (ms) | Newton-Schulz fp64 (ms) |")
	print("|---|---|---|---|---|---|---|")
	for r in rows_out:
		ns = "%.1f (%d it.)" % (r["newton_schulz_ms"], r["newton_schulz_iterations"]) if r["newton_schulz_ms"] is not None else "no convergence in %d it." % r["newton_schulz_iterations"]
		print("| %s | %.3g | %d | %d | %.1f | %.1f | %s |" % (r["block"], r["cond_2"], r["sweeps"], r["pair_launches"], r["svd_ms"], r["numpy_host_ms"], ns))
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
	main()
