"""Dev tool (GPU box): the retrieval chains of consecutive steps on TWO plain streams, paced by the host the way bench.py's partition mode
paces them (step i + 1 is launched once step i - 1 has finished), WITHOUT the exact scan and its CU-masked stream -- rocprofv3 dies in its
finaliser when the process has created one (scripts/r5/step_timeline.sh), so the bench itself cannot be traced in that mode.  What the
trace of this probe answers: once the sweep leaves registers free (DESIGN.md 4.1 'Register account'), does the dispatcher place the next
chain's gather_cols_kernel workgroups beside resident score16_kernel workgroups of the other queue?

  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/gather_beside_sweep_probe.py [--steps 200] [--streams 2]
  python scripts/trace_gather_overlap.py DIR/.../run_kernel_trace.csv 50

cfg2's shape (Q = 10000, I = 100000, 256 anchors, k = 100) on Gaussian operands; prints the host-side ms per step as one JSON line."""
import argparse, json, os, sys, time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anncur_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--streams", type=int, default=2, choices=[1, 2])
ap.add_argument("--Q", type=int, default=10000)
ap.add_argument("--I", type=int, default=100000)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--leading", action="store_true", help="pass leading_sample=True: the plan that sweeps the sampled tiles last (score16.hpp)")
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
Q, I, Kp, k = args.Q, args.I, 256, args.k
A = torch.empty((Q, I), dtype=torch.bfloat16, device=dev)
for r in range(0, Q, 1000):   # (2 GB of bf16: drawn in fp32 slabs)
	A[r:r + 1000] = torch.randn((min(1000, Q - r), I), generator=g, device=dev).to(torch.bfloat16)
anc = torch.randperm(I, generator=g, device=dev)[:Kp].sort().values.to(torch.int32)
Etp = ops.pack_bf16(torch.randn((I, Kp), generator=g, device=dev), Kp, row_multiple=32)
exact_idx = torch.randint(0, I, (Q, k), generator=g, device=dev).to(torch.int32)
cells = [(t, k) for t in (1, 10, 50, 100)]
streams = [torch.cuda.Stream(device=dev) for _ in range(args.streams)]
streams = [streams[s % args.streams] for s in range(2)]
wss = [ops.fused_workspace(Q, I, Kp, k, dev) for _ in range(2)]
done = [torch.cuda.Event() for _ in range(2)]
plan = ops.fused_plan(Q, I, Kp, k, leading_sample=args.leading)
assert plan["lg"] == 1 and plan["ladder"], plan


def chain(slot):
	with torch.cuda.stream(streams[slot]):
		Xq = ops.gather_cols(A, anc)
		top = ops.score_topk_fused(Xq, Etp, I, k, workspace=wss[slot], leading_sample=args.leading)
		ops.overlap_counts(exact_idx, top.indices, cells)
		done[slot].record(streams[slot])


def run(n):
	pending = None
	for i in range(n):
		chain(i & 1)
		if pending is not None:
			while not done[pending].query(): pass
		pending = i & 1
	while not done[pending].query(): pass


torch.cuda.synchronize()
run(args.warmup)
torch.cuda.synchronize()
t0 = time.perf_counter()
run(args.steps)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / args.steps
print(json.dumps({"probe": "gather_beside_sweep", "streams": args.streams, "steps": args.steps, "ms_per_step": round(ms, 4), "lib": os.environ.get("ANNCUR_LIB") or "tree"}))
