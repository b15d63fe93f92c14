"""SparseIPIndex, build_flat_or_ivff_index on sparse input, harness.run_eval_method_embeds and entry point B's tfidf method on .npz files,
each against the DENSE route on the densified matrices.  Integer data throughout: every inner product is exact in fp32, so the dense
route's summation order cannot matter and values and ids must be identical."""
import json
import logging
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
	assert torch.cuda.is_available()
	rng = np.random.default_rng(12)
	items = sn.zipf_csr(rng, 2100, 90, 14, integer=True)
	queries = sn.integer_csr(rng, 9, 90, 0, 30)
	return queries, items, sn.densify(queries), sn.densify(items)


def _same(got, want, what):
	assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[0].shape == want[0].shape, what
	assert np.array_equal(got[1], want[1]), f"{what}: ids differ"
	assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: values differ"


def _rows(m, lo, hi):
	return sn.csr_from_rows([(m.indices[m.indptr[i]:m.indptr[i + 1]], m.data[m.indptr[i]:m.indptr[i + 1]]) for i in range(lo, hi)], m.shape[1])


def test_search_equals_the_flat_index_on_the_densified_matrices(case):
	from anncur_amd.nearest_nbr import FlatIPIndex, SparseIPIndex
	queries, items, dq, di = case
	flat = FlatIPIndex(90)
	flat.add(di)
	sp = SparseIPIndex(90)
	sp.add(items)
	sp.train(None)
	assert sp.ntotal == flat.ntotal == 2100 and sp.search_route(9, 10) == "sparse" and sp.nprobe == 1
	for k in (1, 10, 100, 2048):
		_same(sp.search(queries, k), flat.search(dq, k), f"k={k}")
	# dense queries are sparsified on the way in; a triple is taken as it is
	_same(sp.search(dq, 10), flat.search(dq, 10), "dense queries")
	_same(sp.search(queries.triple, 10), flat.search(dq, 10), "triple queries")
	# k > ntotal: the padding slots hold (-FLT_MAX, -1) on both
	small_f, small_s = FlatIPIndex(90), SparseIPIndex(90)
	small_f.add(di[:7])
	small_s.add(_rows(items, 0, 7))
	got, want = small_s.search(queries, 10), small_f.search(dq, 10)
	_same(got, want, "k > ntotal")
	assert (got[1][:, 7:] == -1).all() and (got[0][:, 7:] == np.finfo(np.float32).min).all() and (got[1][:, :7] >= 0).all()


def test_add_in_two_pieces_equals_add_once(case):
	from anncur_amd.nearest_nbr import SparseIPIndex
	queries, items, _, _ = case
	once, twice = SparseIPIndex(90), SparseIPIndex(90)
	once.add(items)
	twice.add(_rows(items, 0, 777))
	assert twice.ntotal == 777
	_same(twice.search(queries, 5), SparseIPIndex_search_first(items, queries, 777, 5), "after the first piece")
	twice.add(_rows(items, 777, 2100).triple)              # the second piece as a bare triple: the postings are rebuilt at the next search
	assert twice.ntotal == 2100
	_same(twice.search(queries, 100), once.search(queries, 100), "two pieces")


def SparseIPIndex_search_first(items, queries, n, k):
	from anncur_amd.nearest_nbr import SparseIPIndex
	idx = SparseIPIndex(items.shape[1])
	idx.add(_rows(items, 0, n))
	return idx.search(queries, k)


def test_build_flat_or_ivff_index_on_sparse_and_dense_input(case, caplog):
	from anncur_amd.nearest_nbr import FlatIPIndex, SparseIPIndex, build_flat_or_ivff_index
	queries, items, dq, di = case
	sp = build_flat_or_ivff_index(items, False)
	assert isinstance(sp, SparseIPIndex) and sp.ntotal == 2100 and sp.d == 90
	flat = build_flat_or_ivff_index(di, False)
	assert type(flat) is FlatIPIndex                     # dense input: today's path
	_same(sp.search(queries, 64), flat.search(dq, 64), "built indexes")
	assert isinstance(build_flat_or_ivff_index(items.triple, True, n_terms=90), SparseIPIndex)
	with pytest.raises(ValueError, match="dtype = bf16 not supported"):
		build_flat_or_ivff_index(items, False, dtype="bf16")
	# above 11 000 vectors a dense input would take the IVF branch; sparse input stays exact and says so
	rng = np.random.default_rng(1)
	big = sn.integer_csr(rng, 11001, 16, 0, 5)
	with caplog.at_level(logging.INFO, logger="anncur_amd.nearest_nbr"):
		idx = build_flat_or_ivff_index(big, False)
	assert isinstance(idx, SparseIPIndex) and idx.ntotal == 11001
	assert sum("stays exact" in r.getMessage() for r in caplog.records) == 1
	q = sn.integer_csr(rng, 3, 16, 1, 8)
	D, I = idx.search(q, 20)
	ref = sn.densify(q).astype(np.int64) @ sn.densify(big).astype(np.int64).T
	for r in range(3):
		order = np.lexsort((np.arange(11001), -ref[r]))[:20]
		assert np.array_equal(I[r], order) and np.array_equal(D[r], ref[r, order].astype(np.float32))


def test_hard_negative_mining_shape(case):
	"""utils/data_process.py:393-397: k = n_negs + 1 candidates, the gold entity dropped.  Here the gold id goes into exclude=."""
	from anncur_amd.nearest_nbr import FlatIPIndex, SparseIPIndex
	queries, items, dq, di = case
	sp, flat = SparseIPIndex(90), FlatIPIndex(90)
	sp.add(items)
	flat.add(di)
	n_negs = 10
	first = sp.search(queries, 1)[1][:, 0]
	gold = [[int(g)] for g in first]                       # the best item of each query plays the gold entity
	D, I = sp.search(queries, n_negs, exclude=gold)
	assert I.shape == (9, n_negs) and (I >= 0).all() and not (I == first[:, None]).any()
	_same((D, I), flat.search(dq, n_negs, exclude=gold), "exclude the gold id")
	D1, I1 = sp.search(queries, n_negs + 1)
	assert np.array_equal(I1[:, 1:], I) and np.array_equal(I1[:, 0], first)


def _score_matrix(n_test, n_ent, seed):
	g = torch.Generator().manual_seed(seed)
	return torch.randn(n_test, n_ent, generator=g)


def test_harness_returns_the_same_metrics_for_sparse_and_densified_embeddings(case):
	from anncur_amd import harness, ops
	_, items, _, di = case
	rng = np.random.default_rng(5)
	ments = sn.integer_csr(rng, 40, 90, 1, 30)
	A = _score_matrix(40, 2100, 3).cuda()
	grids = {"top_k_vals": [1, 10], "top_k_retr_vals": [20, 100], "n_ent_anchors_vals": [30, 45]}
	dm, de = torch.as_tensor(sn.densify(ments)).cuda(), torch.as_tensor(di).cuda()
	want = harness.run_eval_method_embeds(A, dm, de, 50, grids)
	assert want and harness.run_eval_method_embeds(A, ments, items, 50, grids) == want
	assert harness.run_eval_method_embeds(A, dm, items, 50, grids) == want          # one side dense: it is sparsified
	assert harness.run_eval_method_embeds(A, ments, de, 50, grids) == want
	assert harness.run_eval_method_embeds(A, ops.sparse_csr(ments), ops.sparse_csr(items), 50, grids) == want


def _save_npz(path, m):
	# the layout of scipy.sparse.save_npz, written with numpy alone
	np.savez_compressed(path, indices=m.indices, indptr=m.indptr.astype(np.int32), format="csr".encode("ascii"), shape=np.array(m.shape, dtype=np.int64), data=m.data)


def test_entry_point_B_tfidf_on_npz_files_writes_the_same_json(case, tmp_path):
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	_, items, _, di = case
	n_ent, n_train, n_test = 2100, 20, 60
	rng = np.random.default_rng(8)
	ments = sn.integer_csr(rng, n_train + n_test, 90, 1, 30)        # embeddings of ALL mentions: the entry point takes the test rows (splits.py:378)
	A = _score_matrix(n_train + n_test, n_ent, 4)

	def dump(path, scores, ment_idxs):
		d = {"ment_to_ent_scores": scores, "ment_to_ent_scores.shape": tuple(scores.shape), "test_data": [], "mention_tokens_list": [[0] * 4] * scores.shape[0],
			 "entity_id_list": np.arange(scores.shape[1]), "entity_tokens_list": [], "arg_dict": {}, "ment_idxs": ment_idxs}
		with open(path, "wb") as f:
			pickle.dump(d, f)

	dump(str(tmp_path / "train.pkl"), A[:n_train], list(range(n_train)))
	dump(str(tmp_path / "test.pkl"), A[n_train:], list(range(n_train, n_train + n_test)))
	_save_npz(str(tmp_path / "ment.npz"), ments)
	_save_npz(str(tmp_path / "ent.npz"), items)
	np.save(str(tmp_path / "ment.npy"), sn.densify(ments))
	np.save(str(tmp_path / "ent.npy"), di)
	common = ["--data_name", "lego", "--test_data_file", str(tmp_path / "test.pkl"), "--train_data_file", str(tmp_path / "train.pkl"), "--n_seeds", "1",
			  "--top_k_vals", "1,10", "--top_k_retr_vals", "20,100", "--n_ent_anchors_vals", "30,45", "--eval_method", "tfidf", "--misc", "t"]

	def run(name, ment, ent):
		f = epB.main(common + ["--res_dir", str(tmp_path / name), "--mention_embeds_file", str(tmp_path / ment), "--entity_embeds_file", str(tmp_path / ent)])
		with open(f) as fin:
			return json.load(fin)

	def without_paths(d):     # the three arguments that differ between the runs by construction
		d = json.loads(json.dumps(d))
		for key in ("res_dir", "mention_embeds_file", "entity_embeds_file"):
			assert key in d["other_args"]
			del d["other_args"][key]
		return d

	dense = run("out_dense", "ment.npy", "ent.npy")
	sparse = run("out_npz", "ment.npz", "ent.npz")
	mixed = run("out_mixed", "ment.npy", "ent.npz")
	assert set(sparse) == set(dense) and "seed=0" in dense and dense["seed=0"]
	assert sparse["seed=0"] == dense["seed=0"] and mixed["seed=0"] == dense["seed=0"]
	assert without_paths(sparse) == without_paths(dense)
