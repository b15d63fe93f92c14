#!/usr/bin/env python
"""Timings of the pivoted anchor selection for DESIGN 4.4f (a record, not a gate), by the method of the tables in 4.4c - 4.4e: one process, HIP
events, each timed call queued behind two untimed ones, median of 7 with the minimum in brackets, ms per call.  cfg2's index shape: R
[500 x 100 000] (rank 32 + 0.3 noise), bf16 and fp32.

    python scripts/pivot_probe.py [--out FILE.json]

  * ops.select_pivoted(R, k) for k = 64 / 256 / 500, beside its byte yardstick k kq m b bytes at the 6.29 TB/s copy rate (each step reads R
    once; R fits the 256 MiB Infinity Cache, which may beat the yardstick) and beside the two launches per step it queues;
  * the index build it joins, CURRowIndex(R, anchors) on k random anchors -- unchanged code --, in the same process (the build has host work,
    e.g. the host pseudo-inverse of a square block, so this one is wall time around a synchronisation, same repetition scheme).
Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

REPS = 7
COPY_RATE = 6.29e12   # bytes / s, the measured copy rate


def timed(fn, wall=False):
	"""ms of fn(): REPS times (two untimed calls, then the timed one) -> (median, minimum).  wall: host clock around a synchronisation."""
	ms = []
	for _ in range(REPS):
		fn()
		fn()
		if wall:
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			fn()
			torch.cuda.synchronize()
			ms.append((time.perf_counter() - t0) * 1e3)
			continue
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
	ap.add_argument("--m", type=int, default=100000)
	ap.add_argument("--kq", type=int, default=500)
	ap.add_argument("--ks", type=str, default="64,256,500")
	ap.add_argument("--no_index", action="store_true", help="skip the CURRowIndex builds")
	args = ap.parse_args()
	assert torch.cuda.is_available(), "pivot_probe needs a GPU"
	from anncur_amd import ops
	from anncur_amd.cur import CURRowIndex
	m, kq = args.m, args.kq
	dev = torch.device("cuda:0")
	g = torch.Generator(device=dev).manual_seed(0)
	rank, noise = 32, 0.3
	R32 = torch.randn((kq, rank), generator=g, device=dev) @ torch.randn((rank, m), generator=g, device=dev) / rank ** 0.5 \
		+ noise * torch.randn((kq, m), generator=g, device=dev)
	out = {"m": m, "kq": kq, "reps": REPS}
	for name, R in (("bf16", R32.bfloat16()), ("fp32", R32)):
		for k in [int(x) for x in args.ks.split(",")]:
			med, lo = timed(lambda: ops.select_pivoted(R, k))
			n_sel = ops.select_pivoted(R, k)[2]
			yard = k * kq * m * R.element_size() / COPY_RATE * 1e3
			key = f"select_pivoted {name} k={k}"
			out[key] = {"ms": [round(med, 3), round(lo, 3)], "n_sel": n_sel, "yardstick_ms": round(yard, 3), "us_per_step": round(med / k * 1e3, 2)}
			print(f"{key}: {med:.3f} ({lo:.3f}) ms, n_sel = {n_sel}, {med / k * 1e3:.1f} us per step; k kq m b at 6.29 TB/s = {yard:.3f} ms", flush=True)
			if not args.no_index:
				anc = np.sort(np.random.default_rng(1).choice(m, k, replace=False))
				med, lo = timed(lambda: CURRowIndex(R, anc), wall=True)
				out[f"CURRowIndex {name} k={k}"] = [round(med, 3), round(lo, 3)]
				print(f"CURRowIndex {name} {k} random anchors: {med:.3f} ({lo:.3f}) ms wall", flush=True)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(out, f, indent=1)


if __name__ == "__main__":
	main()
