"""The host side of the far-layout suite (DESIGN "Operands beyond 32-bit offsets"), without a GPU:
  1. the arithmetic of tests/far_layouts.py -- the three properties its docstring promises, for rows in {5, 67, 3000};
  2. the size gates of the sources at their boundaries, through the C entry points: the last accepted value is not refused for that reason,
     the first refused one is refused with its message.  Every call below returns before anything is launched: the gate under test sits in
     front of the workspace check, and the calls carry no workspace (accepted values end there, ANNCUR_E_WORKSPACE) or a shape the next check
     refuses.  Pointers that are only compared with NULL / tested for alignment are dummies.
Gates that are switches between two kernels and not refusals are asserted through the host queries that report the route
(anncur_ivf_search_tile, the plan words); the `buf` switch of the row scans (I x size < 2^31, csrc/topk.hip) has no host query and is NOT
asserted here: it is covered on the device, on both sides, by
tests/test_gpu_kernels.py::test_rowwise_topk_rows_of_2gb_and_more_take_the_pointer_loads.  (10 tests, 2.5 s, no GPU.)
Mutation tried on a scratch build (never committed): plan_wide without its capg loop -- test_row_scan_and_wide_plan_limits fails (capacity
16 384, a span of 2 x 2^32 bytes); the other nine tests pass."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_layouts as fl  # noqa: E402

PTR = 0x10000   # non-null, 256-byte aligned, never dereferenced
LIMIT = 8_421_504   # the last pitch (a multiple of 8) with 255 x pitch x 2 + 64 < 2^32


@pytest.fixture(scope="module")
def lib():
	from anncur_amd import _lib
	return _lib.load()


# ------------------------------------------------------------------ 1. the helper
@pytest.mark.parametrize("misalign", [0, 3])
@pytest.mark.parametrize("rows", [5, 67, 3000])
def test_far_rows_arithmetic(rows, misalign):
	pitch = fl.far_pitch(rows, misalign)
	cols = 4099
	n, start = fl.far_footprint(rows, cols, misalign)
	off = [r * pitch for r in range(rows)]                     # element offsets of the row starts from the view's first element
	assert any(1 << 31 <= o < 1 << 32 for o in off), "no row starts in [2^31, 2^32)"
	assert off[-1] >= 1 << 32, "the last row starts below 2^32"
	assert off[1] < 1 << 31, "no row beside row 0 below 2^31"
	assert pitch % 8 == misalign and start % 8 == misalign and pitch >= cols
	if rows == 5 and not misalign:
		assert pitch == (1 << 30) + 8
	# the guard: every wrapped form of every element a kernel may touch stays inside the allocation
	assert start >= 1 << 31 and n == start + off[-1] + cols
	for o in (off[-1], off[-1] + cols - 1, next(o for o in off if o >= 1 << 31)):
		for es in (2, 4):
			wrapped = [o - (1 << 32) if o < 1 << 32 else o % (1 << 32),                # element offset in 32 bits, signed below 2^32 / unsigned above
					   o % (1 << 32),
					   ((o * es) % (1 << 32)) // es,                                       # byte offset in 32 bits, unsigned
					   (((o * es + (1 << 31)) % (1 << 32)) - (1 << 31)) // es]             # ... and signed
			for w in wrapped:
				assert 0 <= start + w < n, (rows, o, es, w)
	# footprint, as stated: about 6 * 2^30 elements
	assert 6 * (1 << 30) <= n < 6 * (1 << 30) + (1 << 24)
	with pytest.raises(ValueError):
		fl.far_pitch(4)


# ------------------------------------------------------------------ 2. the gates
class _Strided:
	"""What the host predicates of ops read of a bf16 tensor: shape, strides, alignment -- no storage behind it."""
	def __init__(self, shape, ld):
		import torch
		self.shape, self.dtype, self._ld = shape, torch.bfloat16, ld

	def dim(self): return 2
	def stride(self, i): return (self._ld, 1)[i]
	def data_ptr(self): return PTR
	def contiguous(self): return _Strided(self.shape, self.shape[1])


def _score_topk(lib, Kp, ldx, I=70031):
	return lib.anncur_score_topk_ex(PTR, ldx, PTR, Kp, 300, I, Kp, 10, PTR, PTR, None, 0, 0, None, None)


def test_wide_route_refuses_a_query_pitch_beyond_its_32_bit_row_offsets(lib):
	"""wide_query_offsets_fit (csrc/score_fused.hip): wide_kernel's query rows are a 64-bit block base + (row < 256) x ldx x 2 + chunk in 32 bits."""
	for Kp in (640, 1024):
		assert _score_topk(lib, Kp, LIMIT) == -2 and b"workspace" in lib.anncur_last_error()        # accepted: the next thing in the way
		assert _score_topk(lib, Kp, Kp) == -2
		rc = _score_topk(lib, Kp, LIMIT + 8)
		msg = lib.anncur_last_error()
		assert rc not in (0, -2) and b"ldx = 8421512 is too long for the wide kernel's 32-bit row offsets" in msg and b"2^32" in msg, (rc, msg)
	# the Kp <= 512 bodies form qv * ldx in 64 bits: no such limit
	for Kp in (64, 128, 256, 512):
		assert _score_topk(lib, Kp, LIMIT + 8) == -2 and _score_topk(lib, Kp, 1 << 33) == -2
	# (anncur_eval_topk, _timed and anncur_eval_fused go through the same score_topk_impl)
	# the supported-shape queries do not see the pitch
	assert lib.anncur_score_topk_supported(300, 70031, 640, 10) == 1


def test_eval_fused_refuses_an_exact_matrix_pitch_beyond_its_32_bit_tile_offsets(lib):
	"""exact_tile_offsets_fit(lda, 256) in anncur_eval_fused_ex; Q = 0 keeps the accepted call from going on."""
	def call(lda):
		return lib.anncur_eval_fused_ex(PTR, 64, PTR, 64, None, PTR, 1, lda, 0, 40000, 64, 10, PTR, PTR, PTR, PTR, None, 0, None)
	assert call(LIMIT) == 0 or b"outside the fused path" in lib.anncur_last_error()
	rc = call(LIMIT + 8)
	assert rc not in (0, -2) and b"row pitch 8421512 of the exact matrix is too long" in lib.anncur_last_error()
	# ops.eval_fused_ok mirrors the predicate (the harness then takes the two-kernel route), ops._wide_queries the wide one (a compact copy)
	from anncur_amd import ops
	for lda, ok in ((LIMIT, True), (LIMIT + 8, False)):
		assert ops.eval_fused_ok(64, _Strided((300, 40000), lda), 300, 40000, 10) == ok
		for Kp in (640, 1024):
			X = _Strided((300, Kp), lda)
			assert (ops._wide_queries(X) is X) == ok
		X = _Strided((300, 512), lda)
		assert ops._wide_queries(X) is X


def test_ivf_tile128_gate_and_scratch_limit(lib):
	"""ivf_use_tile128 (csrc/ivf.hip): the 128 x 128 bf16 tile kernel forms query and vector addresses as 32-bit byte offsets -- taken only while
	nq x ldq x 2 < 2^32 and 128 x ldx x 2 < 2^32; beyond, the 64-wide tile kernel with 64-bit row pointers.  And the score scratch:
	nq x pitch < 2^32 elements."""
	BF16, F32, T128, GT = 1, 0, lib.anncur_ivf_search_tile(1, 128, 128, 128, 1), lib.anncur_ivf_search_tile(0, 128, 128, 128, 1)
	assert T128 == 128 and GT == 64
	assert lib.anncur_ivf_search_tile(BF16, 128, (1 << 24) - 8, 128, 300) == T128
	assert lib.anncur_ivf_search_tile(BF16, 128, 1 << 24, 128, 300) == GT                          # 128 x 2^24 x 2 = 2^32
	ldq = 8_600_000
	nq_last = ((1 << 31) - 1) // ldq                                                                # nq x ldq < 2^31 elements
	assert nq_last == 249
	assert lib.anncur_ivf_search_tile(BF16, 128, 128, ldq, nq_last) == T128
	assert lib.anncur_ivf_search_tile(BF16, 128, 128, ldq, nq_last + 1) == GT
	assert lib.anncur_ivf_search_tile(BF16, 128, 128, 1 << 23, 256) == GT and lib.anncur_ivf_search_tile(BF16, 128, 128, (1 << 23) - 8, 256) == T128
	assert lib.anncur_ivf_search_tile(BF16, 80, 80, 80, 5) == GT and lib.anncur_ivf_search_tile(F32, 128, 128, 128, 5) == GT

	def search(nq, pitch):
		return lib.anncur_ivf_search_grouped(PTR, F32, 128, 128, PTR, PTR, 4, PTR, 128, nq, PTR, 2, 4, 0, PTR, pitch, None, 0, PTR, PTR, None)
	assert search((1 << 22) - 1, 1024) == -2                                                       # accepted: ends at the missing workspace
	assert search(1 << 22, 1024) == -1 and b"nq * pitch < 2^32" in lib.anncur_last_error()


def test_row_scan_and_wide_plan_limits(lib):
	from anncur_amd import ops
	# int32 item indices: I < 2^31 - 1, refused before any pointer is read
	assert lib.anncur_rowwise_topk(None, 1, 1, (1 << 31) - 1, (1 << 31) - 1, 1, None, None, None) == -1
	assert b"I too large for int32 indices" in lib.anncur_last_error()
	assert lib.anncur_rowwise_topk(None, 1, 1, (1 << 31) - 2, (1 << 31) - 2, 1, None, None, None) == -1
	assert b"null pointer" in lib.anncur_last_error()
	# score_rank's own limit: I < 2^31 - 65 (a 64-item tile past the last id stays inside int32)
	assert lib.anncur_score_rank_workspace_bytes(5, (1 << 31) - 66, 64, 1) > 0 and lib.anncur_score_rank_workspace_bytes(5, (1 << 31) - 65, 64, 1) == 0
	# plan_wide's capg loop: a workgroup's 256 queries x 4 S segments x capacity x 8 bytes stay below 2^32 (32-bit store offsets), whatever k.
	# At its boundary: very many items, k = 2048, few queries -- 64 splits and a capacity the loop halves (from the clamp of 16 384: 2 x 2^32
	# bytes) down to 4096.  The result lies under the limit and one halving fewer would cross it, so a dropped loop fails the first
	# assertion and an over-eager one the second.
	for Q, I, Kp in ((1, 50_000_000, 640), (5, 20_000_000, 1024), (256, 100_000_000, 640)):
		plan = ops.fused_plan(Q, I, Kp, 2048)
		span = 256 * 4 * plan["splits"] * plan["segment_capacity"] * 8
		assert plan["lg"] == 4 and plan["splits"] == 64 and plan["segment_capacity"] == 4096 and span < 1 << 32 <= 2 * span, plan
	for Q, I, k in ((1, 65536 + 17, 2048), (300, 2_000_000, 2048), (1500, 200003, 512), (4096, 1_000_000, 1024), (1, 4_000_000, 2048), (256, 8_000_000, 2048)):
		plan = ops.fused_plan(Q, I, 640, k)
		assert plan["lg"] == 4 and 256 * 4 * plan["splits"] * plan["segment_capacity"] * 8 < 1 << 32, plan
