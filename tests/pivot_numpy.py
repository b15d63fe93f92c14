"""The anchor item selection of include/anncur_hip.h (anncur_select_pivoted) restated in numpy fp64: column-pivoted QR by
twice-applied classical Gram-Schmidt with downdated squared norms, the tie rule (smaller id) and the stop rule (lstsq's pivot rule).  A
helper module, not a test: tests/test_cpu_pivot_host.py holds it against scipy's dgeqp3 and against the closed form below, the GPU tests
hold the kernels against it.  It differs from the device in the ORDER of each sum only (numpy's pairwise / BLAS sums, no fma).

Also here, shared by both: the exact integer data of the GPU tests -- items that are integer multiples of the columns of the n x n Hadamard
matrix, n a power of 4 (64 unless said) -- and the selection it has in closed form."""
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
# the same at the callers' kq: 512 and 600 (the pick kernel's update with two groups and with one), 1027 (its second pass over the rows, a row
# tail of 3 in the step kernel) and 4096 (the limit)
GENERIC_LARGE = [(600, 1500, 48, None, 0.0, 21), (1027, 1200, 40, 30, 0.3, 22), (512, 2000, 64, 40, 0.3, 23), (4096, 700, 24, None, 0.0, 24),
				 # four and three groups in the pick kernel's update (three: uneven shares at every t that is no multiple of 3).  On the exact Hadamard
				 # data every Gram-Schmidt coefficient is 0, so only generic data can tell a wrong update from a right one
				 (256, 1500, 48, None, 0.0, 25), (320, 1500, 47, None, 0.0, 26)]


def hadamard(n=64, dtype=np.int64):
	H = np.ones((1, 1), dtype=dtype)
	while H.shape[0] < n:
		H = np.block([[H, H], [H, -H]])
	assert H.shape[0] == n
	return H


def _power_of_4(n):
	return n >= 1 and n & (n - 1) == 0 and n.bit_length() % 2 == 1


def hadamard_items(scales, kq=64, n=64):
	"""R int64 [kq x m]: item i = scales[i] * H_n[:, i mod n] in the first n rows, zeros in the rows from n on (kq > n makes room for a
	k above the rank n inside the call's limit k <= kq, and for a kq that is no multiple of anything; zero rows change no sum).  n is a power
	of 4, so that 1 / sqrt(n) is a power of two: with |scales| <= 256 every entry is exact in bf16 and fp32, every q_t is +-1/sqrt(n), every
	c_i an exact multiple of sqrt(n) s_i, 0 for an item orthogonal to q_t IN ANY SUMMATION ORDER, and an item parallel to q_t drops to
	d_i = 0 exactly."""
	assert _power_of_4(n) and kq >= n, (n, kq)
	scales = np.asarray(scales, dtype=np.int64)
	R = np.zeros((kq, scales.shape[0]), dtype=np.int64)
	R[:n] = hadamard(n, np.int8)[:, np.arange(scales.shape[0]) % n] * scales[None, :]
	return R


def hadamard_closed_form(scales, k, never=(), n=64):
	"""The selection of hadamard_items(scales, n=n): per direction (i mod n) the item of the largest s^2, the smaller id on a tie; the directions
	in the order of that s^2 descending, then id; gain = n s^2; a direction whose items are all 0 is never reached (d_p = 0 stops).  `never`: ids
	whose columns were overwritten by NaN / inf.  -> (ids int64 [k], gains float64 [k], n_sel).  Two sorts, no loop over the items."""
	assert _power_of_4(n), n
	s2 = np.asarray(scales, dtype=np.int64) ** 2
	ok = s2 > 0
	ok[np.asarray(list(never), dtype=np.int64)] = False
	cand = np.flatnonzero(ok)
	cand = cand[np.lexsort((cand, -s2[cand], cand % n))]          # by direction, then s^2 descending, then id: a direction's winner comes first
	winners = cand[np.r_[True, np.diff(cand % n) != 0]] if cand.size else cand
	winners = winners[np.lexsort((winners, -s2[winners]))]
	ids, gains = np.full(k, -1, dtype=np.int64), np.zeros(k, dtype=np.float64)
	n_sel = min(k, winners.shape[0])
	ids[:n_sel] = winners[:n_sel]
	gains[:n_sel] = float(n) * s2[winners[:n_sel]]
	return ids, gains, n_sel
