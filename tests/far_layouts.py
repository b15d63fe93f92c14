"""Layouts that put a strided operand where 32-bit address arithmetic wraps (no tests and no fixtures here; the arithmetic of far_pitch /
far_footprint is asserted without a GPU in tests/test_cpu_far_layout_host.py).

far_rows: a [rows x cols] view whose row starts, counted in elements from the view's first element, cover all three ranges a kernel's
offset arithmetic can meet:
    row 0 and the rows near it        below 2^31      every 32-bit form is right
    at least one row                  [2^31, 2^32)    a SIGNED 32-bit element offset (int r * ld) is negative here
    at least the last row             >= 2^32         an UNSIGNED 32-bit element offset (uint32_t) wraps here
The pitch is  P = floor8(2^32 / (rows - 1)) + 8  (for 5 rows: 2^30 + 8), a multiple of 8 elements, so the 16-byte vector paths run as on a
compact twin; (rows - 1) P > 2^32 puts the last row past 2^32, and since P < 2^31 the first row at or past 2^31 still starts below
2^31 + P < 2^32.  A byte offset (x 2 or x 4) crosses both lines earlier still.

The allocation is ONE buffer, filled with 0xff bytes over its whole size (NaN as bf16 and as fp32, -1 -- a hole -- as int32 / int16), with a
front guard of GUARD = 2^31 elements before the view.  The guard is what makes a wrong kernel FAIL instead of FAULT:
  - a signed 32-bit wrap of an element offset o in [2^31, 2^32) is o - 2^32 in [-2^31, 0): at most 2^31 elements in front of the view,
    inside the guard;
  - an unsigned 32-bit wrap of o >= 2^32 is o mod 2^32 in [0, o): inside the view's own span (the body);
  - a 32-bit BYTE offset wraps by a multiple of 2^32 bytes: unsigned it lands in the body, signed at most 2^31 bytes <= 2^31 elements in
    front of the view.
In all three cases the kernel reads poison (or another row: the tests give every row its own data) or writes into memory that
assert_only_view_written then finds changed.  Footprint: GUARD + (rows - 1) P + cols, about 6 * 2^30 elements -- 12 GiB of bf16 / int16,
24 GiB of fp32 / int32.

wide_pitch: rows (>= 300, so that row 255 of a 256-row block exists) at a pitch of 8.6 M elements, beyond the 8 421 504 from which
255 rows x pitch x 2 bytes + 64 leaves 32 bits (exact_tile_offsets_fit / wide_query_offsets_fit in csrc/score_fused.hip); 5.2 GB of bf16.
The same poison, no guard: the offsets that wrap there are unsigned byte offsets inside the body."""
import torch

GUARD = 1 << 31
POISON_BYTE = 0xff
_CHUNK = 1 << 27   # int64 words per pass of the poison check (1 GiB)


def far_pitch(rows, misalign=0):
	if rows < 5:
		raise ValueError("far_rows needs rows >= 5")
	return ((1 << 32) // (rows - 1)) // 8 * 8 + 8 + misalign


def far_footprint(rows, cols, misalign=0):
	"""(elements of the allocation, element offset of the view inside it)."""
	start = GUARD + misalign
	return start + (rows - 1) * far_pitch(rows, misalign) + cols, start


def _poisoned(n_elements, dtype, device):
	es = torch.empty((), dtype=dtype).element_size()
	words = -(-n_elements * es // 8)
	raw = torch.empty(words, dtype=torch.int64, device=device)
	raw.fill_(-1)
	return raw.view(dtype)


def far_rows(rows, cols, dtype, device, misalign=0):
	"""(view [rows x cols] of `dtype`, the flat buffer that holds it).  misalign: elements by which the view's first row is moved and the
	pitch lengthened (3: rows lose their 16-byte alignment, each row another one)."""
	pitch = far_pitch(rows, misalign)
	if cols > pitch:
		raise ValueError("far_rows: cols above the pitch")
	n, start = far_footprint(rows, cols, misalign)
	buf = _poisoned(n, dtype, device)
	view = buf.as_strided((rows, cols), (pitch, 1), start)
	return view, buf


def wide_pitch(rows, cols, dtype, device, pitch=8_600_000):
	if rows < 300 or cols > pitch:
		raise ValueError("wide_pitch needs rows >= 300 and cols <= pitch")
	buf = _poisoned((rows - 1) * pitch + cols, dtype, device)
	return buf.as_strided((rows, cols), (pitch, 1), 0), buf


def _int_alias(t):
	return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def repoison(view):
	_int_alias(view).fill_(-1)


def assert_only_view_written(buffer, view, before=None):
	"""For an operand that is an output: everything of `buffer` outside `view` must still be poison.  The view's contents are set aside, the
	view is poisoned, the whole allocation is compared with the poison word by word, and the view gets `before` back (a compact tensor of the
	view's shape: what it held before the call) or stays poison (None).  Take the result out of the view before calling this."""
	repoison(view)
	raw = buffer.view(torch.int64)
	bad = torch.zeros((), dtype=torch.int64, device=buffer.device)
	for s in range(0, raw.numel(), _CHUNK):
		bad += (raw[s:s + _CHUNK] != -1).sum()
	n_bad = int(bad.item())
	if before is not None:
		view.copy_(before)
	assert n_bad == 0, f"{n_bad} 8-byte words outside the view were written"
