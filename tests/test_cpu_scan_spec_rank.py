"""The rank of the exact scan's speculative start (anncur_internal_scan_spec_rank, csrc/topk.hip) against a Poisson tail summed in numpy,
every "off" condition, and the CPU model's restart share on iid rows at the bench shape (scripts/scan_speculation_model.py)."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
N_SEED = {F32: 2048, BF16: 4096}
TAIL = 1e-5   # the library's price of a restart (csrc/topk.hip)


@pytest.fixture(scope="module")
def spec_rank():
	from anncur_amd import _lib
	fn = _lib.load().anncur_internal_scan_spec_rank
	fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int]
	return fn


def _poisson_tail(lam, r):
	"""P[Poisson(lam) >= r] from the upper terms (float64, log-space pmf): no 1 - cdf."""
	j = np.arange(r, r + 4000, dtype=np.float64)
	lg = np.cumsum(np.log(np.arange(1, r + 4000, dtype=np.float64)))          # lg[i] = log((i + 1)!)
	logfact = np.where(j > 0, lg[np.maximum(j.astype(np.int64) - 1, 0)], 0.0)
	return float(np.exp(-lam + j * np.log(lam) - logfact).sum())


def _want(I, k, dtype):
	n = N_SEED[dtype]
	if I < 4 * n:
		return 0
	lam = k * n / I
	for r in range(2, k // 2 + 1):
		if _poisson_tail(lam, r) <= TAIL:
			return r
	return 0


TABLE = [(I, k, dt) for dt in (F32, BF16) for I in (4 * N_SEED[dt] - 1, 4 * N_SEED[dt], 5 * N_SEED[dt] + 5, 40000, 100000, 1000003, 20000000)
		 for k in (1, 2, 3, 4, 5, 8, 10, 16, 50, 64, 65, 100, 128, 129, 512, 2048)]


def test_rank_is_the_smallest_with_the_poisson_tail(spec_rank):
	assert spec_rank(100000, 100, BF16) == 16 and _want(100000, 100, BF16) == 16      # the bench shape
	got = [spec_rank(I, k, dt) for I, k, dt in TABLE]
	want = [_want(I, k, dt) for I, k, dt in TABLE]
	assert got == want, [(c, g, w) for c, g, w in zip(TABLE, got, want) if g != w][:10]
	assert any(w > 0 for w in want) and any(w == 0 for w in want)
	for (I, k, dt), r in zip(TABLE, got):
		if r:
			lam = k * N_SEED[dt] / I
			assert 2 <= r <= k // 2 and _poisson_tail(lam, r) <= TAIL and (r == 2 or _poisson_tail(lam, r - 1) > TAIL)


def test_off_conditions(spec_rank):
	for dt in (F32, BF16):
		n = N_SEED[dt]
		assert spec_rank(4 * n - 1, 100, dt) == 0 and spec_rank(4 * n, 100, dt) > 0            # rows shorter than four seed regions
		assert spec_rank(1025, 100, dt) == 0 and spec_rank(1, 1, dt) == 0
		assert spec_rank(100000, 1, dt) == 0 and spec_rank(100000, 2, dt) == 0 and spec_rank(100000, 3, dt) == 0   # r >= 2 > k / 2
		assert spec_rank(4 * n, 64, dt) == 0 and spec_rank(4 * n, 128, dt) > 0                    # lambda = 16: r = 37 > k / 2
		assert spec_rank(100000, 0, dt) == 0 and spec_rank(100000, -5, dt) == 0
	assert spec_rank(100000, 100, 7) == 0                                                        # not a dtype
	# ANNCUR_SCAN_SPEC=0 (read once per process: a fresh one) turns every shape off; any other value does not
	code = ("import ctypes; from anncur_amd import _lib; f = _lib.load().anncur_internal_scan_spec_rank; f.restype = ctypes.c_int; "
			"f.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int]; print(f(100000, 100, 1), f(100000, 100, 0), f(40000, 128, 1))")
	for val, want in (("0", "0 0 0"), ("1", None), (None, None)):
		env = {k: v for k, v in os.environ.items() if k != "ANNCUR_SCAN_SPEC"}
		if val is not None:
			env["ANNCUR_SCAN_SPEC"] = val
		out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, check=True).stdout.strip()
		assert out == (want or f"{spec_rank(100000, 100, 1)} {spec_rank(100000, 100, 0)} {spec_rank(40000, 128, 1)}"), (val, out)


def test_model_restart_share_at_the_bench_shape():
	spec = importlib.util.spec_from_file_location("scan_speculation_model", os.path.join(ROOT, "scripts", "scan_speculation_model.py"))
	m = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(m)
	r = m.spec_rank(100000, 100, 4096)
	assert r == 16
	assert m.restart_share(1000, 100000, 100, r, 8) <= 1e-2
	# the step-by-step model and the two checks alone agree on which rows restart (a rank low enough to see some)
	rng = np.random.default_rng(3)
	for _ in range(12):
		x = rng.standard_normal(100000, dtype=np.float32)
		c = dict(steps=0, staging_steps=0, staged_vectors=0, drains=0, pushes=0, compactions=0, restarts=0)
		assert m.scan_row(x, 100, 4, 8, c) == (not m.restarts_of(x, 100, 4, 8))
