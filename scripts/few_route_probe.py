"""Small-batch route probe: CURRowIndex.topk for a few queries, small_batch on against off, and off on a build of the parent
commit, in one process.

  python scripts/few_route_probe.py [--parent-lib PATH/libanncur_hip.so] [--reps 21] [--out profiles/few_route_probe.json]

Shapes: Q in {1, 8, 16, 64} at (I = 1e5, Kp = 256, k = 100) and at (I = 1e6, Kp = 512, k = 100).  Every timed call is one HIP-event pair
around ONE call with two untimed calls of the same route in front of it; the routes alternate inside a repetition.  Each shape runs twice:
"resident" on one index over and over (the operand stays in the 256 MiB Infinity Cache where it fits, as a server sees it) and "rotating"
over enough copies of the packed operands to exceed 256 MiB between two uses of a copy, so that the reads come from HBM.
Per shape: ms per call (median and minimum) of each route, the two launches of the new route (launch 1 timed alone through
ops.score_rows_few, launch 2 as the difference of the medians), and the bytes of Et over launch 1's median as a share of 8 TB/s.
--parent-lib: the library of the parent commit; the flag-off call runs on it too (the Python above it is the same: the flag is off)."""
import argparse
import copy
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
from anncur_amd.cur import CURRowIndex  # noqa: E402

SHAPES = [(100_000, 256, 100), (1_000_000, 512, 100)]
QS = (1, 8, 16, 64)
CACHE_BYTES = 256 << 20
PEAK_BYTES_PER_S = 8e12


def _parent_handle(path):
	lib = ctypes.CDLL(path)
	for name, (res, args) in _lib.SIGNATURES.items():
		fn = getattr(lib, name, None)
		if fn is not None:
			fn.restype, fn.argtypes = res, args
	return lib


class _use_lib(object):
	"""Route every ops call to another build of the library for the duration."""

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


def _copies(index, n):
	"""n views of the index whose packed operands are separate allocations."""
	out = [index]
	for _ in range(n - 1):
		c = copy.copy(index)
		c._Etp, c._Etp_sorted, c._item_ids = index._Etp.clone(), index._Etp_sorted.clone(), index._item_ids.clone()
		out.append(c)
	return out


def probe_shape(I, Kp, k, reps, parent):
	g = torch.Generator(device="cuda").manual_seed(I + Kp)
	R = (torch.randn((Kp, I), device="cuda", generator=g) / Kp ** 0.5).bfloat16()
	anc = np.sort(np.random.default_rng(Kp).choice(I, Kp, replace=False))
	on = CURRowIndex(R, anc, compute_dtype="bf16", small_batch=True)
	off = copy.copy(on)
	off.small_batch = False
	et_bytes = on._Etp.numel() * 2
	rows = []
	for mode in ("resident", "rotating"):
		n = 1 if mode == "resident" else CACHE_BYTES // et_bytes + 2
		ons, offs = _copies(on, n), _copies(off, n)
		for Q in QS:
			X = torch.randn((Q, Kp), device="cuda", generator=g).bfloat16()
			Xp = ops.pack_bf16(X, Kp)
			assert on.topk_route(Q, k) == "bf16-few" and off.topk_route(Q, k) != "bf16-few"
			t = {"few": [], "off": [], "parent_off": [], "launch1": []}
			for r in range(reps):
				a, b = ons[r % n], offs[r % n]
				t["few"].append(_timed(lambda: a.topk(X, k)))
				t["off"].append(_timed(lambda: b.topk(X, k)))
				if parent is not None:
					with _use_lib(parent):
						t["parent_off"].append(_timed(lambda: b.topk(X, k)))
				t["launch1"].append(_timed(lambda: ops.score_rows_few(Xp, a._Etp, I)))
			row = {"I": I, "Kp": Kp, "k": k, "Q": Q, "mode": mode, "copies": n, "off_route": off.topk_route(Q, k), "et_bytes": et_bytes}
			for name, ms in t.items():
				if ms:
					row[name] = _stats(ms)
			row["launch2_ms"] = row["few"]["median_ms"] - row["launch1"]["median_ms"]
			row["launch1_share_of_8TBps"] = et_bytes / (row["launch1"]["median_ms"] * 1e-3) / PEAK_BYTES_PER_S
			rows.append(row)
			print(json.dumps(row), flush=True)
		del ons, offs
		torch.cuda.empty_cache()
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--parent-lib", default=None)
	ap.add_argument("--reps", type=int, default=21)
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "few_route_probe.json"))
	ap.add_argument("--shapes", default="all", help="'all', 'small' (I = 1e5 only)")
	ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from (default: HEAD of this checkout)")
	args = ap.parse_args()
	assert args.reps >= 21 or args.shapes != "all", "the table takes the median and minimum of at least 21 calls"
	parent = _parent_handle(args.parent_lib) if args.parent_lib else None
	commit = args.parent_commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
	rows = []
	for I, Kp, k in (SHAPES if args.shapes == "all" else SHAPES[:1]):
		rows += probe_shape(I, Kp, k, args.reps, parent)
	out = {"device": torch.cuda.get_device_name(0), "commit_parent": commit, "parent_lib": bool(parent), "reps": args.reps, "rows": rows}
	os.makedirs(os.path.dirname(args.out), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(out, f, indent=1)
	print("wrote", args.out)


if __name__ == "__main__":
	main()
