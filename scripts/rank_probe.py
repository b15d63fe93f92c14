"""Dev tool (GPU box): the ranks of given items at cfg2 size -- 10 000 queries x 100 000 items, 256 anchor items, bf16 --
with targets = each query's exact top-100.  One process, HIP events, two untimed calls before every timed loop.  Three rows:
  1. index.rank_of(X, exact top-100): the fused route (collect + sort + count + finish), S_hat never written;
  2. the route it replaces for a recall curve up to k_retvr = 1000: index.topk(X, 1000) + ops.overlap_counts;
  3. ops.rank_in_rows over the bf16 exact matrix (the same targets), with the rate at which it streams the matrix.
  python scripts/rank_probe.py [--steps 10]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from anncur_amd import ops
from anncur_amd.cur import CURRowIndex
from anncur_amd.synth import protocol_b

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--Q", type=int, default=10000)
ap.add_argument("--I", type=int, default=100000)
ap.add_argument("--anchors", type=int, default=256)
ap.add_argument("--kq", type=int, default=512)
args = ap.parse_args()
dev = torch.device("cuda")
Q, I, k = args.Q, args.I, 100
A_train, A_test = protocol_b(args.kq, Q, I, dev, seed=0)
anc = sorted(np.random.default_rng(0).choice(I, size=args.anchors, replace=False))
index = CURRowIndex(A_train, np.asarray(anc), compute_dtype="bf16")
X = ops.gather_cols(A_test, anc)
exact = ops.rowwise_topk(A_test, k)
assert index.rank_route(k) == "bf16"


def timed(fn):
	for _ in range(2): fn()
	torch.cuda.synchronize()
	ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
	ev[0].record()
	for _ in range(args.steps): out = fn()
	ev[1].record(); torch.cuda.synchronize()
	return ev[0].elapsed_time(ev[1]) / args.steps, out


cells = [(t, kr) for kr in (100, 200, 500, 1000) for t in (1, 10, 50, 100)]
ms_rank, ranks = timed(lambda: index.rank_of(X, exact.indices))
ms_topk, counts = timed(lambda: ops.overlap_counts(exact.indices, index.topk(X, 1000).indices, cells))
ms_rows, self_ranks = timed(lambda: ops.rank_in_rows(A_test, exact.indices))
assert torch.equal(self_ranks, torch.arange(k, dtype=torch.int32, device=dev).expand(Q, k))   # the exact top-k, ranked in the exact matrix
r = ranks.cpu().numpy()
Kp = index._Etp.shape[1]
print(f"Q={Q} I={I} anchors={args.anchors} (Kp={Kp}) bf16, targets = exact top-{k}, {args.steps} timed calls each")
print(f"  1. index.rank_of (fused, S_hat never written)      {ms_rank:8.3f} ms   = {2.0 * Q * Kp * I / ms_rank / 1e9:.0f} TFLOP/s of tile work; "
	  f"median rank {int(np.median(r))}, p99 {int(np.percentile(r, 99))}, max {int(r.max())}")
print(f"  2. index.topk(X, 1000) + overlap_counts          {ms_topk:8.3f} ms   (the curve up to k_retvr = 1000 only)")
print(f"  3. rank_in_rows over the bf16 exact matrix       {ms_rows:8.3f} ms   = {Q * I * 2 / ms_rows / 1e6:.0f} GB/s")
