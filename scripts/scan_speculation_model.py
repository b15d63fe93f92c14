#!/usr/bin/env python3
"""CPU model of the candidate path of the wave-per-row exact scan (csrc/topk.hip, rowwise_topk_wave_kernel) on iid rows: what the choice of
the FIRST threshold does to the number of times that path runs.

Modelled as the kernel does it: the row in 16-byte vectors, 64 per step, 8 steps per block; the threshold a block filters with is the one at
the block's start; a step in which some vector passes stages those vectors (64-entry staging area, drained when the next step's would not
fit, at the quarter mark of a speculative pass, and at the end); a drain pushes the staged elements that beat the CURRENT threshold; above
`trigger` candidates the buffer is compacted to its k best and the k-th becomes the threshold.  First threshold: the rank-th largest of the
512 group maxima of the first 512 vectors (the bound itself is admitted).  rank = k is a valid bound; rank < k is a guess that is checked --
at the block boundary nearest a quarter of the row (no compaction yet and fewer than k / 8 candidates: restart) and at the row's end (no
compaction and fewer than k: restart) -- and a restart scans the row again at rank k; its steps, drains, pushes and compactions are counted
with the row's.

Not modelled: ties (Gaussian rows have none), the head / tail of a misaligned row, NaN.

  python scripts/scan_speculation_model.py [--rows 300] [--I 100000] [--k 100] [--vec 8] [--ranks 12 10]
prints, per scheme, the per-row means of: steps that stage (of all steps), staged vectors, drains, pushes, compactions, and the rows that
restarted.  The rank the library would choose (anncur_internal_scan_spec_rank's rule, restated here) is always among the schemes."""
import argparse
import math

import numpy as np

STEP_VECS, BLOCK_STEPS, SEED_VECS, STAGE = 64, 8, 512, 64


def spec_rank(I, k, n_seed, tail=1e-5):
	"""Smallest r >= 2 with P[Poisson(k n_seed / I) >= r] <= tail; 0 (off) if r > k / 2 or I < 4 n_seed."""
	if I < 4 * n_seed:
		return 0
	lam = k * n_seed / I
	r = 0
	while 2 * r <= k:
		if r >= 2 and 1.0 - sum(math.exp(-lam + j * math.log(lam) - math.lgamma(j + 1)) for j in range(r)) <= tail:
			return r
		r += 1
	return 0


def trigger(k):
	return min(k + max(k + k // 2, 64), 512)


def seed_threshold(gmax, rank):
	"""Just below the rank-th largest of the seed's group maxima."""
	return np.nextafter(np.partition(gmax[:SEED_VECS], SEED_VECS - rank)[SEED_VECS - rank], np.float32(-np.inf))


def restarts_of(x, k, rank, vec):
	"""Does a speculative pass over the row restart?  (The two checks alone: no step loop.)"""
	nvec = x.size // vec
	tau = seed_threshold(x[:nvec * vec].reshape(nvec, vec).max(axis=1), rank)
	nsteps = -(-nvec // STEP_VECS)
	cp = max(((nsteps // 4 + BLOCK_STEPS // 2) // BLOCK_STEPS) * BLOCK_STEPS, BLOCK_STEPS)
	above = x > tau
	if (cp + 2 * BLOCK_STEPS) * STEP_VECS <= nvec and int(above[:cp * STEP_VECS * vec].sum()) < k // 8:
		return True
	return int(above.sum()) < k


def restart_share(rows, I, k, rank, vec, seed=0):
	rng = np.random.default_rng(seed)
	return sum(restarts_of(rng.standard_normal(I, dtype=np.float32), k, rank, vec) for _ in range(rows)) / rows


def scan_row(x, k, rank, vec, c):
	"""One pass over the row from the rank-th seed maximum; counters added to c.  -> False if the pass restarts."""
	nvec = x.size // vec
	g = x[:nvec * vec].reshape(nvec, vec)
	gmax = g.max(axis=1)
	tau = seed_threshold(gmax, rank)
	spec = rank < k
	trig = trigger(k)
	nsteps = -(-nvec // STEP_VECS)
	cp = max(((nsteps // 4 + BLOCK_STEPS // 2) // BLOCK_STEPS) * BLOCK_STEPS, BLOCK_STEPS) if spec else -1
	buf, staged, compacted = np.empty(0, dtype=np.float32), [], False

	def drain():
		nonlocal buf, staged, tau, compacted
		e = g[np.concatenate(staged)].reshape(-1)
		e = e[e > tau]
		c["pushes"] += e.size
		c["drains"] += 1
		buf = np.concatenate([buf, e])
		staged = []
		if buf.size > trig:
			buf = np.partition(buf, buf.size - k)[buf.size - k:]
			tau = buf.min()
			compacted = True
			c["compactions"] += 1

	tau_blk = tau
	for s in range(nsteps):
		if s % BLOCK_STEPS == 0:
			if s == cp and (cp + 2 * BLOCK_STEPS) * STEP_VECS <= nvec:
				if staged:
					drain()
				if not compacted and buf.size < k // 8:
					return False
			tau_blk = tau
		v = np.flatnonzero(gmax[s * STEP_VECS:(s + 1) * STEP_VECS] > tau_blk) + s * STEP_VECS
		c["steps"] += 1
		if v.size:
			if sum(a.size for a in staged) + v.size > STAGE:
				drain()
			staged.append(v)
			c["staging_steps"] += 1
			c["staged_vectors"] += v.size
	if staged:
		drain()
	tail = x[nvec * vec:]
	buf = np.concatenate([buf, tail[tail > tau]])
	return not (spec and not compacted and buf.size < k)


def model(rows, I, k, rank, vec, seed=0):
	rng = np.random.default_rng(seed)
	c = dict(steps=0, staging_steps=0, staged_vectors=0, drains=0, pushes=0, compactions=0, restarts=0)
	for _ in range(rows):
		x = rng.standard_normal(I, dtype=np.float32)
		if not scan_row(x, k, rank, vec, c):
			c["restarts"] += 1
			assert scan_row(x, k, k, vec, c)
	return c


def main():
	ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
	ap.add_argument("--rows", type=int, default=300)
	ap.add_argument("--I", type=int, default=100000)
	ap.add_argument("--k", type=int, default=100)
	ap.add_argument("--vec", type=int, default=8, help="elements per 16-byte vector: 8 = bf16, 4 = fp32")
	ap.add_argument("--ranks", type=int, nargs="*", default=[12, 10], help="further ranks to model beside k (today) and the library's choice")
	a = ap.parse_args()
	auto = spec_rank(a.I, a.k, SEED_VECS * a.vec)
	schemes = [("k-th largest seed maximum (valid bound)", a.k)]
	if auto:
		schemes.append((f"{auto}th largest (the library's choice)", auto))
	schemes += [(f"{r}th largest seed maximum", r) for r in a.ranks if r not in (a.k, auto) and 1 <= r < a.k]
	print(f"{a.rows} iid Gaussian rows, I = {a.I}, k = {a.k}, {a.vec} elements per vector, trigger {trigger(a.k)}; per-row means")
	print(f"{'first threshold':44s} {'steps that stage':>18s} {'staged vectors':>15s} {'drains':>8s} {'pushes':>8s} {'compactions':>12s} {'rows restarted':>15s}")
	for name, rank in schemes:
		c = model(a.rows, a.I, a.k, rank, a.vec)
		n = a.rows
		print(f"{name:44s} {c['staging_steps'] / n:10.1f} of {c['steps'] / n:4.0f} {c['staged_vectors'] / n:15.1f} {c['drains'] / n:8.2f} {c['pushes'] / n:8.1f} "
			  f"{c['compactions'] / n:12.2f} {c['restarts']:8d} of {n}")


if __name__ == "__main__":
	main()
