"""The anchor item selection of include/anncur_hip.h (anncur_select_pivoted) restated in numpy fp64: column-pivoted QR by
twice-applied classical Gram-Schmidt with downdated squared norms, the tie rule (smaller id) and the stop rule (lstsq's pivot rule).  A
helper module, not a test: tests/test_cpu_pivot_host.py holds it against scipy's dgeqp3 and against the closed form below, the GPU tests
hold the kernels against it.  It differs from the device in the ORDER of each sum only (numpy's pairwise / BLAS sums, no fma).

Also here, shared by both: the exact integer data of the GPU test -- items that are integer multiples of the columns of the 64 x 64 Hadamard
matrix -- and the selection it has in closed form."""
import numpy as np

STOP = 2.0 ** -40


def select(R, k):
	"""-> (ids int64 [k], gains float64 [k], n_sel, gaps float64 [n_sel]).  Positions >= n_sel hold (-1, 0.0).  gaps[t] = (d_best - d_second) /
	d_first of step t over the candidates (inf where step t had one candidate only): how far the argmax was from a different answer."""
	R = np.asarray(R, dtype=np.float64)
	kq, m = R.shape
	ids, gains, gaps = np.full(k, -1, dtype=np.int64), np.zeros(k, dtype=np.float64), []
	with np.errstate(invalid="ignore", over="ignore"):
		d = np.einsum("ai,ai->i", R, R)
		taken = np.zeros(m, dtype=bool)
		basis = np.zeros((0, kq))
		d_first, n_sel = 0.0, 0
		for t in range(k):
			cand = np.isfinite(d) & ~taken                      # NaN and +-inf are never taken
			if not cand.any():
				break
			dm = np.where(cand, d, -np.inf)
			p = int(np.argmax(dm))                               # the first of equal maxima: the smaller id
			dp = float(d[p])
			if t == 0:
				d_first = dp
			if dp <= 0.0 or (t > 0 and dp <= STOP * d_first):
				break
			dm[p] = -np.inf
			gaps.append((dp - dm.max()) / d_first)
			ids[t], gains[t], n_sel = p, dp, t + 1
			v = R[:, p].copy()
			for _ in range(2):                                    # classical Gram-Schmidt, twice
				if t:
					v = v - basis.T @ (basis @ v)
			q = v / np.sqrt(v @ v)
			basis = np.vstack([basis, q[None, :]])
			c = q @ R
			d = d - c * c
			taken[p] = True
	return ids, gains, n_sel, np.asarray(gaps, dtype=np.float64)


def low_rank(kq, m, rank, noise, seed):
	"""rank-`rank` structure plus noise (rank None: a full-rank Gaussian matrix), fp32: the generic shapes of the tests."""
	rng = np.random.default_rng(seed)
	if rank is None:
		return rng.standard_normal((kq, m)).astype(np.float32)
	return (rng.standard_normal((kq, rank)) @ rng.standard_normal((rank, m)) / np.sqrt(rank) + noise * rng.standard_normal((kq, m))).astype(np.float32)


# (kq, m, k, rank, noise, seed): the minimum gap of each is asserted >= 2^-30 before anything is compared against the restatement
GENERIC = [(48, 700, 40, 12, 0.4, 11), (37, 1031, 37, 8, 0.3, 12), (64, 515, 33, None, 0.0, 13)]


def hadamard(n=64):
	H = np.ones((1, 1), dtype=np.int64)
	while H.shape[0] < n:
		H = np.block([[H, H], [H, -H]])
	assert H.shape[0] == n
	return H


def hadamard_items(scales, kq=64):
	"""R int64 [kq x m]: item i = scales[i] * H[:, i mod 64] in the first 64 rows, zeros in the rows from 64 on (kq > 64 makes room for a
	k above the rank 64 inside the call's limit k <= kq; zero rows change no sum).  With |scales| <= 256 every entry is exact in bf16 and
	fp32, every q_t is +-1/8, every c_i an exact multiple of 8 s_i, 0 for an item orthogonal to q_t, and an item parallel to q_t drops to
	d_i = 0 exactly."""
	scales = np.asarray(scales, dtype=np.int64)
	R = np.zeros((kq, scales.shape[0]), dtype=np.int64)
	R[:64] = hadamard(64)[:, np.arange(scales.shape[0]) % 64] * scales[None, :]
	return R


def hadamard_closed_form(scales, k, never=()):
	"""The selection of hadamard_items(scales): per direction (i mod 64) the item of the largest s^2, the smaller id on a tie; the directions in
	the order of that s^2 descending, then id; gain = 64 s^2; a direction whose items are all 0 is never reached (d_p = 0 stops).  `never`: ids
	whose columns were overwritten by NaN / inf.  -> (ids int64 [k], gains float64 [k], n_sel)."""
	s2 = np.asarray(scales, dtype=np.int64) ** 2
	winners = []
	for j in range(64):
		items = [i for i in range(j, s2.shape[0], 64) if i not in never and s2[i] > 0]
		if items:
			winners.append(min(items, key=lambda i: (-s2[i], i)))
	winners.sort(key=lambda i: (-s2[i], i))
	ids, gains = np.full(k, -1, dtype=np.int64), np.zeros(k, dtype=np.float64)
	n_sel = min(k, len(winners))
	ids[:n_sel] = winners[:n_sel]
	gains[:n_sel] = 64.0 * s2[winners[:n_sel]]
	return ids, gains, n_sel
