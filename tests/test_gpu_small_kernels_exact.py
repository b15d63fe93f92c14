"""The small kernels on the GEMMs' path -- anncur_convert (ops.convert, ops.pack_bf16), anncur_gather_cols, anncur_gather_rows
(csrc/topk.hip) -- bit for bit: conversions over every bit pattern against torch's CPU conversion, the gathers against host indexing
at the sizes around their unrolls and launch chunks, and the documented safety net for a bad index held in a device tensor.

No comparison here has a tolerance.  Sources are interior views of larger NaN-filled buffers wherever a kernel could read past an
edge: a wrong read stays inside the test's own allocation and shows up as NaN.  Device-side bad indices are -1, n and n + 1 only.
Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

F32, BF16 = torch.float32, torch.bfloat16
LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)   # below / at / above the rounding tie, both ends


@pytest.fixture(scope="module")
def ops():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	from anncur_amd import ops as _ops
	return _ops


def _bits16(t):
	return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits32(t):
	return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _interior(x, dtype=None, top=2, left=3, bottom=3, right=4):
	"""Host tensor [R x C] -> device view holding it inside a NaN-filled buffer (padded pitch, rows and columns of NaN all round)."""
	R, C = x.shape
	buf = torch.full((R + top + bottom, C + left + right), float("nan"), dtype=dtype or x.dtype, device=DEV)
	v = buf[top:top + R, left:left + C]
	v.copy_(x)
	return v


def _ragged(patterns, n_cols, np_dtype):
	"""1-D array of bit patterns -> [rows x n_cols] with zero patterns filling the last row."""
	rows = -(-patterns.size // n_cols)
	full = np.zeros(rows * n_cols, dtype=np_dtype)
	full[:patterns.size] = patterns
	return full.reshape(rows, n_cols)


# ------------------------------------------------------------------ convert over bit patterns
def test_convert_f32_to_bf16_over_every_upper_half(ops):
	"""All 65536 upper halves x six lower halves: ties to even, rounding up into the next exponent, overflow to inf, denormals, zeros
	and infinities must equal torch's CPU conversion bit for bit; a NaN stays a NaN of the same sign (the kernel quiets the payload,
	torch canonicalises it)."""
	up = np.arange(65536, dtype=np.uint32)
	pat = np.concatenate([(up << 16) | lo for lo in LOW_HALVES]).astype(np.uint32)
	src_bits = _ragged(pat, 517, np.uint32)   # 517 columns: three workgroups per row, the last one ragged
	src = torch.from_numpy(src_bits.view(np.int32)).view(F32)
	got = _bits16(ops.convert(_interior(src), BF16))
	want = _bits16(src.bfloat16())
	nan = np.isnan(src_bits.view(np.float32))
	assert nan.sum() == 6 * 2 * 127 + 2 * 5 and (~nan).sum() > 390000
	assert np.array_equal(got[~nan], want[~nan])
	assert ((got[nan] & 0x7fff) > 0x7f80).all() and np.array_equal(got[nan] >> 15, (src_bits[nan] >> 31).astype(np.uint16))
	# the data does what the case is about: ties (both parities), carries into the exponent, overflow to inf, denormal inputs
	x = src_bits[~nan]
	w = want[~nan]
	tie = (x & 0xffff) == 0x8000
	assert (tie & ((x >> 16) & 1 == 0)).any() and (tie & ((x >> 16) & 1 == 1)).any()
	assert ((w & 0x7f80) != ((x >> 16) & 0x7f80).astype(np.uint16)).any()
	assert (((w & 0x7fff) == 0x7f80) & ((x & 0x7fffffff) < 0x7f800000)).any()
	assert (((x & 0x7f800000) == 0) & ((x & 0x7fffff) != 0)).any()


def test_convert_bf16_to_f32_over_every_pattern(ops):
	pat = np.arange(65536, dtype=np.uint16)
	src_bits = _ragged(pat, 261, np.uint16)
	src = torch.from_numpy(src_bits.view(np.int16)).view(BF16)
	got = _bits32(ops.convert(_interior(src), F32))
	assert np.array_equal(got, src_bits.astype(np.uint32) << 16)   # NaN payloads included: the conversion is a shift


@pytest.mark.parametrize("src_dtype", [F32, BF16])
def test_convert_more_rows_than_one_launch_takes(ops, src_dtype):
	"""65535 + 3 rows: the row-chunk loop inside anncur_convert (grid.y limit)."""
	n = 65535 + 3
	x = (torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) * 0.37 - 1000.0).to(src_dtype)
	for dst_dtype in (F32, BF16):
		got = ops.convert(_interior(x), dst_dtype).cpu()
		assert got.shape == (n, 3) and got.dtype == dst_dtype
		assert torch.equal(got, x.to(dst_dtype))


# ------------------------------------------------------------------ pack_bf16
@pytest.mark.parametrize("src_dtype", [F32, BF16])
@pytest.mark.parametrize("n,K,Kp,row_multiple", [(1, 64, 64, 32), (32, 1, 64, 32), (33, 37, 64, 32), (33, 128, 128, 1), (70, 300, 512, 32), (5, 1, 64, 1)])
def test_pack_bf16_values_and_exact_zero_padding(ops, n, K, Kp, row_multiple, src_dtype):
	g = torch.Generator().manual_seed(n * 1000 + K)
	x = (torch.randn(n, K, generator=g) * 100).to(src_dtype)
	n_pad = -(-n // row_multiple) * row_multiple
	want = np.zeros((n_pad, Kp), dtype=np.uint16)
	want[:n, :K] = _bits16(x.bfloat16())
	# a column slice of a wider NaN-filled matrix (row pitch, neighbours that must not leak into the padding), and a plain source
	for src in (_interior(x), x.to(DEV)):
		got = ops.pack_bf16(src, Kp, row_multiple=row_multiple)
		assert got.shape == (n_pad, Kp) and got.dtype == BF16 and got.is_contiguous()
		assert np.array_equal(_bits16(got), want)   # values, and +0.0 bit for bit in the row and column padding


# ------------------------------------------------------------------ gathers
N_IDX = (0, 1, 63, 64, 65, 255, 256, 257)   # around gather_cols' unroll of 64 lanes x 4


def _index_list(n_idx, n, seed):
	"""Unsorted, with duplicates, with negative (wrapping) entries, touching both ends of the dimension."""
	rng = np.random.default_rng(seed)
	idx = rng.integers(-n, n, size=n_idx)
	if n_idx >= 4:
		idx[:4] = (n - 1, -n, 0, -1)
	if n_idx >= 8:
		idx[5] = idx[6] = idx[2]
	return [int(i) for i in idx]


@pytest.mark.parametrize("dst_dtype", [F32, BF16])
@pytest.mark.parametrize("src_dtype", [F32, BF16])
@pytest.mark.parametrize("n_idx", N_IDX)
def test_gather_cols_and_rows_host_index_lists(ops, n_idx, src_dtype, dst_dtype):
	R, C = 9, 301
	x = (torch.randn(R, C, generator=torch.Generator().manual_seed(n_idx)) * 50).to(src_dtype)
	cols = _index_list(n_idx, C, 1)
	if n_idx >= 8:
		assert min(cols) < 0 and len(set(cols)) < len(cols) and cols != sorted(cols)
	for src in (_interior(x), x.to(DEV)):
		got = ops.gather_cols(src, cols, out_dtype=dst_dtype)
		assert got.shape == (R, n_idx) and got.dtype == dst_dtype
		assert torch.equal(got.cpu(), x[:, cols].to(dst_dtype))
	xt = x.t().contiguous()   # [301 x 9]: the same list as row indices
	for src in (_interior(xt), xt.to(DEV)):
		got = ops.gather_rows(src, cols, out_dtype=dst_dtype)
		assert got.shape == (n_idx, R) and got.dtype == dst_dtype
		assert torch.equal(got.cpu(), xt[cols, :].to(dst_dtype))
	# numpy arrays and CPU tensors are host index lists as well
	if n_idx:
		assert torch.equal(ops.gather_cols(x.to(DEV), np.asarray(cols)).cpu(), x[:, cols])
		assert torch.equal(ops.gather_rows(xt.to(DEV), torch.tensor(cols)).cpu(), xt[cols, :])


@pytest.mark.parametrize("C", [1, 255, 256, 257, 600])
def test_gather_rows_wide_rows(ops, C):
	"""gather_rows walks a row in workgroups of 256 columns."""
	x = torch.randn(7, C, generator=torch.Generator().manual_seed(C))
	rows = [6, -7, 3, 3, 0, -1]
	for dst_dtype in (F32, BF16):
		assert torch.equal(ops.gather_rows(_interior(x), rows, out_dtype=dst_dtype).cpu(), x[rows, :].to(dst_dtype))


def test_gather_rows_more_indices_than_one_launch_takes(ops):
	"""65535 + 3 indices into a small matrix: the chunk loop in ops.gather_rows (grid.y limit); the last three rows come from the
	second launch."""
	x = torch.randn(37, 5, generator=torch.Generator().manual_seed(0))
	idx = np.random.default_rng(0).integers(-37, 37, size=65535 + 3)
	idx[-3:] = (36, -37, 5)
	got = ops.gather_rows(_interior(x), idx)
	assert got.shape == (65538, 5) and torch.equal(got.cpu(), x[torch.from_numpy(idx)])
	got = ops.gather_rows(_interior(x.bfloat16()), idx.tolist(), out_dtype=F32)
	assert torch.equal(got.cpu(), x.bfloat16().float()[torch.from_numpy(idx)])


@pytest.mark.parametrize("bad", [[0, 5, 301], [-302, 1], [2 ** 31], [-2 ** 31 - 1, 0]])
def test_gathers_raise_index_error_for_host_indices_out_of_range(ops, bad):
	x = torch.zeros(301, 301, device=DEV)
	for fn in (ops.gather_cols, ops.gather_rows):
		for idx in (bad, np.asarray(bad), torch.tensor(bad)):
			with pytest.raises(IndexError):
				fn(x, idx)


@pytest.mark.parametrize("dst_dtype", [F32, BF16])
@pytest.mark.parametrize("src_dtype", [F32, BF16])
def test_bad_device_index_yields_zero_and_reads_nothing(ops, src_dtype, dst_dtype):
	"""The documented safety net: an index held in a DEVICE tensor is not checked on the host, and the kernels write 0 for one outside
	[0, n).  Only -1, n and n + 1 are used, and the matrix is an interior view of a NaN-filled buffer with room on every side: an
	unclamped read would land inside that buffer and come back as NaN."""
	R, C = 6, 70
	x = (torch.randn(R, C, generator=torch.Generator().manual_seed(1)) * 10).to(src_dtype)
	for n, fn, dim in ((C, ops.gather_cols, 1), (R, ops.gather_rows, 0)):
		idx = [0, -1, n - 1, n, 3, n + 1, 3, -1]
		src = _interior(x, top=2, left=3, bottom=3, right=4)   # rows / columns -1, n and n + 1 of the view all exist in the buffer
		got = fn(src, torch.tensor(idx, dtype=torch.int32, device=DEV), out_dtype=dst_dtype).cpu()
		ok = torch.tensor([0 <= i < n for i in idx])
		good = torch.tensor([i if 0 <= i < n else 0 for i in idx])
		want = x.index_select(dim, good).to(dst_dtype)
		mask = ok.view(1, -1) if dim == 1 else ok.view(-1, 1)
		want = torch.where(mask, want, torch.zeros((), dtype=dst_dtype))
		assert not torch.isnan(got.float()).any()
		assert torch.equal(got.view(torch.int32 if dst_dtype == F32 else torch.int16), want.view(torch.int32 if dst_dtype == F32 else torch.int16))   # +0.0, bit for bit
		# an int64 device tensor takes the same path
		got64 = fn(src, torch.tensor(idx, dtype=torch.int64, device=DEV), out_dtype=dst_dtype).cpu()
		assert torch.equal(got64, want)
