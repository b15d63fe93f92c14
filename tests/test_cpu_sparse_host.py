"""Host side of the sparse inner-product route (no GPU): the numpy model (tests/sparse_numpy.py) against the int64 dense product,
the proof that its data make the summation order visible, the host validation of ops.sparse_postings / sparse_score_topk / sparse_csr, the
plan at its boundaries, the C ABI's new symbols, the kernel's resource numbers and the .npz reader."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_numpy as sn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"anncur_sparse_score_rows": 14, "anncur_sparse_score_topk": 15, "anncur_sparse_score_topk_workspace_bytes": 3, "anncur_sparse_plan": 4}


def _model_data(kind):
	rng = np.random.default_rng(20)
	gen = sn.integer_csr if kind == "int" else sn.real_csr
	return gen(rng, 5, 300, 20, 89), gen(rng, 4101, 300, 1, 39)


# ------------------------------------------------------------------ the model
def test_scores_ref_equals_the_int64_dense_product_on_integer_data():
	queries, items = _model_data("int")
	want = sn.densify(queries).astype(np.int64) @ sn.densify(items).astype(np.int64).T
	got = sn.scores_ref(queries, items)
	assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want) and np.abs(want).max() < 1 << 24
	assert not (got.view(np.uint32) == 0x80000000).any()                       # +0.0, never -0.0
	assert np.array_equal(sn.scores_ref(queries, items, descending=True).view(np.uint32), got.view(np.uint32))   # integers: any order


def test_the_summation_order_is_visible_in_the_real_valued_data():
	queries, items = _model_data("real")
	up, down = sn.scores_ref(queries, items), sn.scores_ref(queries, items, descending=True)
	differ = int((up.view(np.uint32) != down.view(np.uint32)).sum())
	print("scores that differ between ascending and descending chains:", differ, "of", up.size)
	assert up.size == 20505 and differ >= 1
	np.testing.assert_allclose(up, sn.densify(queries).astype(np.float64) @ sn.densify(items).astype(np.float64).T, rtol=0, atol=1e-4)


def test_postings_ref_and_group_maxima():
	items = sn.csr_from_rows([([0, 2], [1, 2]), ([], []), ([2], [3]), ([1, 2], [4, 5])], 4)
	term_ptr, post_item, post_val = sn.postings_ref(items)
	assert term_ptr.tolist() == [0, 1, 2, 5, 5] and post_item.tolist() == [0, 3, 0, 2, 3] and post_val.tolist() == [1, 4, 2, 3, 5]
	S = np.arange(130, dtype=np.float32)[None, :].copy()
	S[0, 64] = np.nan
	assert sn.group_maxima(S).tolist() == [[63.0, 127.0, 129.0]]


# ------------------------------------------------------------------ ops: validation before any device
def _triple(rows, V):
	m = sn.csr_from_rows(rows, V)
	return m.indptr, m.indices, m.data


def _fake_postings(n, V):
	from anncur_amd import ops
	return ops.SparsePostings(torch.zeros(V + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float32), n, V)


def test_sparse_postings_validates_on_the_host():
	from anncur_amd import ops
	good = [([0, 3], [1, 2]), ([1, 2, 4], [1, 1, 1]), ([], [])]
	with pytest.raises(ValueError, match=r"row 1 .*unsorted, term 1 follows term 2.*sort_indices"):
		ops.sparse_postings(*_triple([good[0], ([2, 1, 4], [1, 1, 1])], 5), 2, 5)
	with pytest.raises(ValueError, match=r"row 2 .*duplicate term 4.*sum_duplicates"):
		ops.sparse_postings(*_triple([good[0], good[1], ([4, 4], [1, 1])], 5), 3, 5)
	with pytest.raises(ValueError, match=r"term id -1 is outside \[0, 5\)"):
		ops.sparse_postings(*_triple([([-1, 3], [1, 2])], 5), 1, 5)
	with pytest.raises(ValueError, match=r"term id 5 is outside \[0, 5\)"):
		ops.sparse_postings(*_triple([([0, 5], [1, 2])], 5), 1, 5)
	ip, ix, d = _triple(good, 5)
	with pytest.raises(ValueError, match=r"indptr must start at 0 .*indptr\[0\] = 1"):
		ops.sparse_postings(ip + 1, ix, d, 3, 5)
	bad = ip.copy()
	bad[-1] = 4
	with pytest.raises(ValueError, match=r"end at nnz = 5 .*indptr\[-1\] = 4"):
		ops.sparse_postings(bad, ix, d, 3, 5)
	with pytest.raises(ValueError, match="indptr decreases at row 1"):
		ops.sparse_postings(np.array([0, 3, 2, 5], dtype=np.int64), ix, d, 3, 5)
	with pytest.raises(ValueError, match=r"expected n_items \+ 1 = 5"):
		ops.sparse_postings(ip, ix, d, 4, 5)
	with pytest.raises(TypeError, match=r"indptr int64, indices int32, data float32"):
		ops.sparse_postings(ip.astype(np.int32), ix, d, 3, 5)
	with pytest.raises(TypeError, match=r"indptr int64, indices int32, data float32"):
		ops.sparse_postings(ip, ix.astype(np.int64), d, 3, 5)
	with pytest.raises(TypeError, match=r"indptr int64, indices int32, data float32"):
		ops.sparse_postings(ip, ix, d.astype(np.float64), 3, 5)
	with pytest.raises(ValueError, match=r"V = 2147483648 terms, the limit is V < 2\^31"):
		ops.sparse_postings(ip, ix, d, 3, 1 << 31)
	with pytest.raises(ValueError, match="at least one item"):
		ops.sparse_postings(np.zeros(1, dtype=np.int64), ix[:0], d[:0], 0, 5)
	c = ops.sparse_csr((ip, ix, d), 5, "x")      # rows [0, 3] and [1, 2, 4]: a row may start below the end of the one before it
	assert (c.n_rows, c.n_cols) == (3, 5)


def test_sparse_score_topk_validates_on_the_host():
	from anncur_amd import _lib, ops
	post = _fake_postings(1000, 50)
	q = _triple([([0, 3], [1, 2])], 50)
	for k, pat in ((0, r"k = 0 outside 1\.\.min\(n, ANNCUR_MAX_TOPK\) = min\(1000, 2048\) = 1000"), (1001, r"k = 1001 outside")):
		with pytest.raises(ValueError, match=pat):
			ops.sparse_score_topk(q, post, k)
	with pytest.raises(ValueError, match=r"k = 2049 outside .* = 2048"):
		ops.sparse_score_topk(q, _fake_postings(5000, 50), 2049)
	with pytest.raises(ValueError, match=r"row 0 is not in canonical form: unsorted"):
		ops.sparse_score_topk(_triple([([3, 0], [1, 2])], 50), post, 10)
	with pytest.raises(ValueError, match=r"term id 50 is outside \[0, 50\)"):
		ops.sparse_score_topk(_triple([([0, 50], [1, 2])], 50), post, 10)
	big = _fake_postings(1000, 5000)
	n = ops.SPARSE_MAX_QNNZ
	assert n == _lib.SPARSE_MAX_QNNZ == 1024
	long_q = _triple([([1], [1.0]), (np.arange(n + 1), np.ones(n + 1))], 5000)
	with pytest.raises(ValueError, match=r"row 1 stores 1025 terms, above ANNCUR_SPARSE_MAX_QNNZ = 1024"):
		ops.sparse_score_topk(long_q, big, 10)
	with pytest.raises(ValueError, match=r"row 1 stores 1025 terms"):
		ops.sparse_score_rows(long_q, big)
	obj = sn.csr_from_rows([([0, 3], [1, 2])], 49)
	with pytest.raises(ValueError, match=r"the matrix has 49 columns, expected 50"):
		ops.sparse_score_topk(obj, post, 10)
	with pytest.raises(TypeError, match="expected a CSR operand"):
		ops.sparse_score_topk(np.zeros((2, 50), dtype=np.float32), post, 10)
	with pytest.raises(TypeError, match=r"indptr int64, indices int32, data float32"):
		ops.sparse_score_topk((q[0], q[1], q[2].astype(np.float64)), post, 10)
	with pytest.raises(TypeError, match="postings must come from sparse_postings"):
		ops.sparse_score_topk(q, (post.term_ptr, post.post_item, post.post_val), 10)
	with pytest.raises(_lib.AnncurHipError):            # valid arguments on CPU tensors: there is no CPU path
		ops.sparse_score_topk(q, post, 10)
	with pytest.raises(_lib.AnncurHipError):
		ops.sparse_score_rows(q, post)


def test_duck_typed_csr_objects_are_converted_and_triples_are_strict():
	from anncur_amd import ops
	m = sn.csr_from_rows([([0, 3], [1, 2]), ([], []), ([1], [0.5])], 5)
	scipy_like = sn.CSR(m.indptr.astype(np.int32), m.indices, m.data.astype(np.float64), m.shape)     # what scipy / sklearn hand over
	c = ops.sparse_csr(scipy_like, what="x")
	assert (c.indptr.dtype, c.indices.dtype, c.data.dtype) == (torch.int64, torch.int32, torch.float32) and (c.n_rows, c.n_cols) == (3, 5)
	assert c.indptr.tolist() == [0, 2, 2, 3] and c.data.tolist() == [1.0, 2.0, 0.5]
	assert ops.is_sparse_arg(scipy_like) and ops.is_sparse_arg(m.triple) and ops.is_sparse_arg(c)
	assert not ops.is_sparse_arg(np.zeros((3, 5), dtype=np.float32)) and not ops.is_sparse_arg(torch.zeros(3, 5)) and not ops.is_sparse_arg([np.zeros(4)] * 3)
	csc = sn.CSR(m.indptr, m.indices, m.data, m.shape)
	csc.format = "csc"
	with pytest.raises(TypeError, match="csc format, CSR is required"):
		ops.sparse_csr(csc, what="x")
	d = ops.sparse_from_dense(sn.densify(m))
	assert d.indptr.tolist() == [0, 2, 2, 3] and d.indices.tolist() == [0, 3, 1] and d.data.tolist() == [1.0, 2.0, 0.5] and d.n_cols == 5


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("Q", [1, 64, 10000])
@pytest.mark.parametrize("I", [1, 2048, 2049, 100000])
def test_sparse_plan_at_its_boundaries(Q, I):
	from anncur_amd import _lib, ops
	p = ops.sparse_plan(Q, I)
	W = -(-I // 2048)
	assert p["windows"] == W and p["groups"] == -(-I // 64) and p["pitch"] == -(-I // 32) * 32 and p["max_qnnz"] == 1024
	assert p["waves_per_workgroup"] == 4 and p["lds_bytes"] == 1024 * 8 + 4 * (2048 * 4 + 1024 * 8) == 73728 and 2 * p["lds_bytes"] <= 160 * 1024
	wpw = min(W, -(-Q * W // 2048))                   # about 2048 waves in all, a wave never less than one window
	assert p["windows_per_wave"] == wpw and p["spans"] == -(-W // wpw) and p["workgroups_per_query"] == -(-p["spans"] // 4)
	assert p["workgroups"] == Q * p["workgroups_per_query"]
	assert (p["spans"] - 1) * wpw < W <= p["spans"] * wpw          # every window has exactly one owner, the last span is not empty
	assert _lib.load().anncur_sparse_score_topk_workspace_bytes(Q, I, 1) == Q * p["pitch"] * 4


def test_sparse_plan_examples_and_limits():
	from anncur_amd import _lib, ops
	assert ops.sparse_plan(1, 100000)["windows_per_wave"] == 1 and ops.sparse_plan(1, 100000)["workgroups"] == 13        # one query spreads over its 49 windows
	assert ops.sparse_plan(10000, 100000)["windows_per_wave"] == 49 and ops.sparse_plan(10000, 100000)["workgroups"] == 10000
	assert ops.sparse_plan(65, 81925)["windows_per_wave"] == 2                                                           # the shape the GPU test uses for the hand-over
	lib = _lib.load()
	assert lib.anncur_sparse_score_topk_workspace_bytes(4, 1000, 1001) == 0 and lib.anncur_sparse_score_topk_workspace_bytes(4, 1000, 0) == 0
	assert lib.anncur_sparse_score_topk_workspace_bytes(0, 1000, 1) == 0 and lib.anncur_sparse_score_topk_workspace_bytes(4, (1 << 31) - 1, 1) == 0
	for Q, I in ((0, 10), (1, 0), (1, (1 << 31) - 1)):
		with pytest.raises(ValueError, match="sparse_plan"):
			ops.sparse_plan(Q, I)
	assert ops.sparse_plan(1, (1 << 31) - 2)["windows"] == 1 << 20


# ------------------------------------------------------------------ the built library
def test_new_symbols_are_declared_and_exported():
	from anncur_amd import _lib
	lib = _lib.load()
	src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "anncur_hip.h")).read(), flags=re.S)
	for name, n_args in NEW_SYMBOLS.items():
		m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
		assert m and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args == len(m.group(1).split(",")), name
	assert "#define ANNCUR_SPARSE_WINDOW 2048" in src and "#define ANNCUR_SPARSE_MAX_QNNZ 1024" in src and "#define ANNCUR_SPARSE_PLAN_WORDS 10" in src


def test_sparse_kernel_uses_no_scratch():
	"""From the built library's metadata (resource numbers only): the scoring kernel spills nothing, and its registers leave room for the
	eight waves per SIMD that two 72 KB workgroups per CU never reach (LDS is dynamic: the static size is 0)."""
	sys.path.insert(0, os.path.join(ROOT, "scripts"))
	from check_kernel_resources import parse_kernel_notes
	from isa_tools import kernel_notes
	from anncur_amd import _lib
	kernels = [k for text in kernel_notes(_lib.LIB_PATH) for k in parse_kernel_notes(text) if "sparse" in k[".name"]]
	assert [k for k in kernels if "sparse_score_kernel" in k[".name"]] and len(kernels) == 1, [k[".name"] for k in kernels]
	for k in kernels:
		assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
		assert not k.get(".uses_dynamic_stack", False) and k[".vgpr_count"] <= 64 and k[".group_segment_fixed_size"] == 0


def test_sparse_kernel_multiplies_and_adds_in_two_instructions():
	"""The contract is two roundings per step.  hipcc once fused the step into v_fmac_f32 (through __fmul_rn / __fadd_rn, which do not prevent
	it) and a third of the real-valued scores were off by an ulp on the device; the built kernel must hold no fused fp32 multiply-add."""
	sys.path.insert(0, os.path.join(ROOT, "scripts"))
	from isa_tools import disassemble, functions
	from anncur_amd import _lib
	bodies = [body for dis in disassemble(_lib.LIB_PATH) for name, body in functions(dis) if "sparse_score_kernel" in name and not name.endswith(".kd")]
	assert len(bodies) == 1 and len(bodies[0]) > 100
	ops_seen = [ins.split()[0] for _, ins, _ in bodies[0]]
	fused = [o for o in ops_seen if re.match(r"v_(fma|fmac|mac|mad|pk_fma)\w*_f32", o)]
	assert not fused, fused
	assert sum(o.startswith("v_mul_f32") for o in ops_seen) >= 1 and sum(o.startswith("v_add_f32") for o in ops_seen) >= 1


# ------------------------------------------------------------------ .npz embeddings
def test_load_embeds_reads_save_npz_layout_without_scipy(tmp_path):
	from anncur_amd import harness, ops
	m = sn.csr_from_rows([([0, 3], [1, 2]), ([], []), ([1, 4], [0.5, -1])], 5)
	path = str(tmp_path / "ent.npz")
	np.savez_compressed(path, indices=m.indices, indptr=m.indptr.astype(np.int32), format="csr".encode("ascii"), shape=np.array(m.shape), data=m.data.astype(np.float64))
	before = set(sys.modules)
	c = harness.load_embeds(path)
	assert not any(name.split(".")[0] == "scipy" for name in set(sys.modules) - before)
	assert isinstance(c, ops.SparseCSR) and (c.n_rows, c.n_cols) == (3, 5) and c.indptr.tolist() == [0, 2, 2, 4] and c.indices.tolist() == [0, 3, 1, 4]
	assert c.data.dtype == torch.float32 and c.data.tolist() == [1.0, 2.0, 0.5, -1.0] and c.indptr.dtype == torch.int64
	t = harness.take_embed_rows(c, [2, 0, 2])
	assert t.indptr.tolist() == [0, 2, 4, 6] and t.indices.tolist() == [1, 4, 0, 3, 1, 4] and t.data.tolist() == [0.5, -1.0, 1.0, 2.0, 0.5, -1.0] and t.n_rows == 3
	np.save(str(tmp_path / "ent.npy"), sn.densify(m))
	assert np.array_equal(harness.load_embeds(str(tmp_path / "ent.npy")), sn.densify(m))
	np.savez(str(tmp_path / "csc.npz"), indices=m.indices, indptr=m.indptr, format=b"csc", shape=np.array(m.shape), data=m.data)
	with pytest.raises(ValueError, match="sparse format csc"):
		harness.load_embeds(str(tmp_path / "csc.npz"))
	np.savez(str(tmp_path / "bad.npz"), indices=m.indices[::-1].copy(), indptr=m.indptr, format=b"csr", shape=np.array(m.shape), data=m.data)
	with pytest.raises(ValueError, match="not in canonical form"):
		harness.load_embeds(str(tmp_path / "bad.npz"))
