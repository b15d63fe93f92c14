"""The two drop-in CLIs end to end on synthetic pickles laid out like the reference's inputs, checked against the goldens
generated from the reference, plus the flat inner-product index.  Needs an MI355X."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


def _dump(path, scores, **extra):
	os.makedirs(os.path.dirname(path), exist_ok=True)
	d = {"ment_to_ent_scores": scores, "ment_to_ent_scores.shape": tuple(scores.shape), "test_data": [], "mention_tokens_list": [[0] * 4] * scores.shape[0],
		 "entity_id_list": np.arange(scores.shape[1]), "entity_tokens_list": [], "arg_dict": {}}
	d.update(extra)
	with open(path, "wb") as f:
		pickle.dump(d, f)


def test_entry_point_A_cli_matches_reference_goldens(gpu, tmp_path, golden_meta):
	"""BASELINE config 1 shape: 1k x 5k fp32, 64 anchors, k=10 through run_retrieval_eval_wrt_exact_crossenc.py."""
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from utils.zeshel_utils import score_matrix_filename
	torch.manual_seed(0)
	A = torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)
	res_dir = str(tmp_path / "res")
	_dump(score_matrix_filename(res_dir, "yugioh", 1000), A)
	out_dir = epA.main(["--data_name", "yugioh", "--res_dir", res_dir, "--n_ment", "1000", "--n_seeds", "2", "--disable_wandb", "1", "--misc", "t",
						"--eval_methods", "cur,cur_oracle", "--n_ment_anchors_vals", "64,128", "--n_ent_anchors_vals", "64",
						"--top_k_vals", "10", "--top_k_retr_vals", "100,6000"])
	assert out_dir.endswith("yugioh/Retrieval_wrt_Exact_CrossEnc/nm=1000_ne=5000_s=2_t")
	with open(os.path.join(out_dir, "retrieval_wrt_exact_crossenc.json")) as f:
		res = json.load(f)
	assert set(res) == {"cur", "cur_oracle", "other_args"}
	assert res["other_args"]["n_ment_anchors_vals"] == [64, 128] and res["other_args"]["arg_dict"]["data_name"] == "yugioh"
	assert "k_retvr=6000" not in res["cur"]["top_k=10"]                      # k_retvr > n_ent cells are skipped like the reference
	gold = golden_meta["entryA"]["results"]
	cell = res["cur_oracle"]["top_k=10"]["k_retvr=100"]["anc_n_m=64~anc_n_e=64"]
	for t in ("anchor", "non_anchor", "all"):
		for m, v in gold["cur_oracle_2seeds"][t].items():
			assert cell[t][m] == pytest.approx(v, rel=2e-3, abs=2e-3), (t, m)
	cell = res["cur"]["top_k=10"]["k_retvr=100"]["anc_n_m=128~anc_n_e=64"]    # over-sampled anchors: well conditioned
	for t in ("anchor", "non_anchor", "all"):
		for m, v in gold["cur_kq128_ki64_2seeds"][t].items():
			tol = 2e-2 if ("_p50" in m or "_std" in m) else 3e-3
			assert cell[t][m] == pytest.approx(v, rel=tol, abs=tol), (t, m)
	assert os.path.isdir(os.path.join(out_dir, "plots_non_anchor"))


def _tight(metric, top_k):
	"""Tolerance of the --pinv numpy runs: U is bit-identical to the reference's, only the GEMMs' summation order differs.
	Means to 1e-4 (the reference rounds its own numbers to 4 decimals; count means are top_k x the fractions), p50 to one count, the
	standard deviations to 1e-3, the Frobenius errors to 1e-4 relative."""
	frac = "_frac_" in metric
	if metric.endswith("_p50"):
		return dict(abs=(1.0 / top_k if frac else 1.0) + 1e-9)
	if metric.endswith("_std"):
		return dict(abs=1e-3 if frac else 1e-3 * top_k)
	if metric.endswith("_mean"):
		return dict(abs=1.0001e-4 if frac else 1.0001e-4 * top_k)
	return dict(rel=1e-4)


def test_entry_point_A_cli_with_numpy_pinv_matches_reference_goldens_to_1e4(gpu, tmp_path, golden_meta):
	"""The one setting in which the drop-in claim is exact: --pinv numpy (the reference's own numpy.linalg.pinv call on the host).  Same
	run as above; every metric of both cells -- the well-conditioned cur cell AND cur_oracle -- against the reference's goldens at the
	reference's own resolution."""
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from utils.zeshel_utils import score_matrix_filename
	torch.manual_seed(0)
	A = torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)
	res_dir = str(tmp_path / "res")
	_dump(score_matrix_filename(res_dir, "yugioh", 1000), A)
	out_dir = epA.main(["--data_name", "yugioh", "--res_dir", res_dir, "--n_ment", "1000", "--n_seeds", "2", "--disable_wandb", "1", "--misc", "np",
						"--eval_methods", "cur,cur_oracle", "--n_ment_anchors_vals", "64,128", "--n_ent_anchors_vals", "64",
						"--top_k_vals", "10", "--top_k_retr_vals", "100", "--pinv", "numpy"])
	with open(os.path.join(out_dir, "retrieval_wrt_exact_crossenc.json")) as f:
		res = json.load(f)
	assert res["other_args"]["arg_dict"]["pinv"] == "numpy"
	gold = golden_meta["entryA"]["results"]
	for method, cell_key, gkey in (("cur_oracle", "anc_n_m=64~anc_n_e=64", "cur_oracle_2seeds"), ("cur", "anc_n_m=128~anc_n_e=64", "cur_kq128_ki64_2seeds")):
		cell = res[method]["top_k=10"]["k_retvr=100"][cell_key]
		for t in ("anchor", "non_anchor", "all"):
			for m, v in gold[gkey][t].items():
				tol = _tight(m, 10)
				if m.startswith("approx_error"):
					# the reference's torch.norm accumulates 4.7 M squares in fp32 and comes out 1.06e-4 LOW of the float64 value of its own
					# S_hat - A (measured with the oracle in this container: 424.2436 vs 424.2885); this build sums per row and then in
					# float64 -- the accurate value, checked against the oracle's float64 norm below -- so the golden is met to 2.5e-4
					tol = dict(rel=2.5e-4)
				assert cell[t][m] == pytest.approx(v, **tol), (method, t, m, cell[t][m], v)
	# ... and the accurately summed error norm to 2e-5: the oracle's S_hat (fp32, as the reference computes it), its error norm in float64
	from oracle import cur_oracle as O
	want = []
	for seed in range(2):
		rng = np.random.default_rng(seed)
		ri = sorted(rng.choice(1000, 128, replace=False)); ci = sorted(rng.choice(5000, 64, replace=False))
		o = O.CURApproxOracle(rows=A[ri, :], cols=A[:, ci], row_idxs=ri, col_idxs=ci, approx_preference="rows")
		non = sorted(set(range(1000)) - set(int(i) for i in ri))
		want.append(float((o.get(list(range(1000)), list(range(5000))) - A)[non, :].double().norm()))
	got = res["cur"]["top_k=10"]["k_retvr=100"]["anc_n_m=128~anc_n_e=64"]["non_anchor"]["approx_error"]
	assert got == pytest.approx(np.mean(want), rel=2e-5), (got, want)


def test_entry_point_B_cli_with_numpy_pinv_matches_reference_sweep_to_1e4(gpu, tmp_path, golden_meta):
	"""Entry point B with --pinv numpy against the reference's own sweep (same inputs as the test below): means to 1e-4, p50 to one count."""
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	res_file = epB.main(["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
						 "--train_data_file", str(tmp_path / "train.pkl"), "--n_seeds", "6", "--misc", "np",
						 "--top_k_vals", "1,10,50,100", "--top_k_retr_vals", "5,10,50", "--n_ent_anchors_vals", "10,20,30", "--pinv", "numpy"])
	with open(res_file) as f:
		got = json.load(f)["seed=5"]
	n_checked = 0
	for key, v in golden_meta["entryB_sweep"]["results"].items():
		tk, kr, na = key.split("|")
		cell = got[tk][kr][f"anc_n_m=60_{na}"]
		for m, want in v.items():
			assert cell[m] == pytest.approx(want, **_tight(m, int(tk.split("=")[1]))), (key, m, cell[m], want)
			n_checked += 1
	assert n_checked > 100


def test_entry_A_single_seed_square_anchor_case(gpu, golden_meta):
	"""Kq == Ki = 64: the intersection is square and ill-conditioned (the reference's own rel. error is 1.46); anchor rows are still
	reproduced and the recall agrees to a few 1e-3."""
	from anncur_amd import harness
	torch.manual_seed(0)
	A = torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)
	got = harness.run_approx_eval_w_seed("cur", A.cuda(), 64, 64, 10, 100, 0)
	gold = golden_meta["entryA"]["results"]["cur_seed0"]
	key = "exact_vs_reranked_approx_retvr~common_frac_mean"
	assert got["anchor"][key] == pytest.approx(1.0)
	assert got["all"][key] == pytest.approx(gold["all"][key], abs=1e-2)
	assert got["non_anchor"][key] == pytest.approx(gold["non_anchor"][key], abs=1e-2)
	assert float(got["all"]["approx_error_relative"]) == pytest.approx(gold["all"]["approx_error_relative"], rel=5e-2)
	empty = harness.run_approx_eval_w_seed("cur", A[:64].cuda(), 64, 32, 10, 100, 0)   # every row is an anchor: non_anchor is empty
	assert np.isnan(float(empty["non_anchor"]["approx_error_relative"])) and empty["non_anchor"][key] == 0.0


def test_entry_point_B_cli_matches_reference_sweep(gpu, tmp_path, golden_meta):
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	# the reference consumes rng(5) sequentially over the anchor counts 10, 20, 30 -> seed 5 == 6th seed of a 6-seed run
	res_file = epB.main(["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
						 "--train_data_file", str(tmp_path / "train.pkl"), "--n_seeds", "6", "--misc", "sweep",
						 "--top_k_vals", "1,10,50,100", "--top_k_retr_vals", "5,10,50", "--n_ent_anchors_vals", "10,20,30"])
	assert res_file.endswith("method=cur_sweep.json")
	with open(res_file) as f:
		res = json.load(f)
	assert set(res) == {f"seed={s}" for s in range(6)} | {"other_args"}
	assert res["other_args"]["retriever_params"]["n_ent_anchors_vals"] == [10, 20, 30]
	got = res["seed=5"]
	gold = golden_meta["entryB_sweep"]["results"]
	for key, v in gold.items():
		tk, kr, na = key.split("|")
		cell = got[tk][kr][f"anc_n_m=60_{na}"]
		for m, want in v.items():
			tol = (1.0 if "frac" not in m else 0.11) if m.endswith("_p50") else (0.06 if "frac" not in m else 6e-3)   # a near-tie may move one count
			assert cell[m] == pytest.approx(want, abs=tol), (key, m)
	assert "k_retvr=5" not in got.get("top_k=10", {})


def test_default_grids_match_reference(gpu):
	from anncur_amd import harness
	gB = harness.default_grids_B(10031, "cur")
	assert gB["top_k_vals"] == [1, 10, 50, 100] and 900 in gB["top_k_retr_vals"] and gB["top_k_retr_vals"][0] == 0
	assert 10031 in gB["n_ent_anchors_vals"] and 2000 in gB["n_ent_anchors_vals"]
	assert harness.default_grids_B(10031, "bienc")["top_k_retr_vals"] == [1, 10, 50, 100, 200, 500, 1000]
	gA = harness.default_grids_A(3374, 10031)
	assert gA["n_ment_anchors_vals"] == [50, 100, 200, 500, 1000, 2000] and gA["n_ent_anchors_vals"][-1] == 10031
	assert gA["top_k_vals"] == [10] and gA["top_k_retr_vals"] == [500] and gA["eval_methods"] == ["cur", "cur_oracle"]


@pytest.mark.parametrize("n,d,nq,k,dtype", [(3000, 96, 37, 10, "fp32"), (12000, 768, 20, 64, "fp32"), (70000, 128, 50, 100, "bf16"), (50, 16, 5, 64, "fp32"),
											   (30000, 768, 300, 64, "bf16")])   # d = 768 bi-encoder embeddings in bf16: the K-general fused kernel
def test_flat_ip_index_matches_exact_search(gpu, n, d, nq, k, dtype):
	from models.nearest_nbr import build_flat_or_ivff_index
	from oracle import cur_oracle as O
	g = np.random.default_rng(n)
	X = g.standard_normal((n, d)).astype(np.float32); q = g.standard_normal((nq, d)).astype(np.float32)
	if dtype == "bf16":
		X = torch.tensor(X).bfloat16().float().numpy(); q = torch.tensor(q).bfloat16().float().numpy()
	index = build_flat_or_ivff_index(torch.tensor(X), force_exact_search=n > 11000, dtype=dtype)   # (above 11 000 the default is IVF-flat)
	D, I = index.search(q, k)
	assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (nq, k)
	rD, rI = O.flat_ip_search(X, q, min(k, n))
	np.testing.assert_allclose(D[:, :min(k, n)], rD, rtol=1e-4, atol=1e-4)
	common = np.mean([len(set(a) & set(b)) / len(b) for a, b in zip(I[:, :min(k, n)].tolist(), rI.tolist())])
	assert common > 0.999
	if k > n:
		assert (I[:, n:] == -1).all() and (D[:, n:] == np.finfo(np.float32).min).all()


def test_ivf_flat_index_branch(gpu):
	"""models/nearest_nbr.py:40-52: above 11 000 vectors the reference builds IndexIVFFlat(nlist = floor(sqrt(n)), nprobe =
	floor(sqrt(nlist) * mult)).  FAISS is absent (parity unpinned): the GPU index is checked for its defining properties and
	judged on recall against the exact search."""
	from models.nearest_nbr import build_flat_or_ivff_index
	from anncur_amd.nearest_nbr import IVFFlatIPIndex, FlatIPIndex
	from oracle import cur_oracle as O
	g = np.random.default_rng(7)
	n, d, nq, k = 40000, 96, 200, 10
	centers = g.standard_normal((64, d)).astype(np.float32) * 2                      # clustered data, like entity embeddings
	X = (centers[g.integers(0, 64, n)] + g.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
	q = (centers[g.integers(0, 64, nq)] + g.standard_normal((nq, d)).astype(np.float32)).astype(np.float32)
	index = build_flat_or_ivff_index(X, force_exact_search=False)
	assert isinstance(index, IVFFlatIPIndex) and index.nlist == 200 and index.nprobe == 14 and index.ntotal == n and index.is_trained
	assert isinstance(build_flat_or_ivff_index(X, force_exact_search=True), FlatIPIndex)
	assert isinstance(build_flat_or_ivff_index(X[:11000], force_exact_search=False), FlatIPIndex)
	assert build_flat_or_ivff_index(X, False, probe_mult_factor=2).nprobe == 28
	D, I = index.search(q, k)
	assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (nq, k) and (I >= 0).all()
	assert (D[:, :-1] >= D[:, 1:]).all()
	np.testing.assert_allclose(D, np.take_along_axis(q @ X.T, I, axis=1), rtol=1e-5, atol=1e-4)   # reported scores are the true inner products
	# every list is complete and disjoint; the search equals a brute-force search restricted to the probed lists
	off, ids = index._offsets.cpu().numpy(), index._ids.cpu().numpy()
	assert off[0] == 0 and off[-1] == n and (np.sort(ids) == np.arange(n)).all()
	C = index.centroids.cpu().numpy()
	assign = np.empty(n, dtype=np.int64)
	for l in range(index.nlist):
		assign[ids[off[l]:off[l + 1]]] = l
	assert (np.argmax(X @ C.T, axis=1) == assign).mean() > 0.999                       # each vector sits in its max-inner-product list (fp32 near-ties aside)
	probe = np.argsort(-(q @ C.T), axis=1)[:, :index.nprobe]
	for j in range(0, nq, 17):
		cand = np.concatenate([ids[off[l]:off[l + 1]] for l in probe[j]])
		want = cand[np.argsort(-(X[cand] @ q[j]), kind="stable")[:k]]
		assert len(set(want.tolist()) & set(I[j].tolist())) >= k - 1                   # (a boundary near-tie may swap)
	# recall against the exact search, and exact equality when every list is probed
	rD, rI = O.flat_ip_search(X, q, k)
	recall = np.mean([len(set(a) & set(b)) / k for a, b in zip(I.tolist(), rI.tolist())])
	assert recall > 0.9, recall
	index.nprobe = index.nlist
	D2, I2 = index.search(q, k)
	np.testing.assert_allclose(D2, rD, rtol=1e-5, atol=1e-4)
	assert np.mean([len(set(a) & set(b)) / k for a, b in zip(I2.tolist(), rI.tolist())]) > 0.999
	# FAISS convention when the probed lists hold fewer than k vectors: (-inf, -1) padding
	index.nprobe = 1
	D3, I3 = index.search(q[:4], 1000)
	sizes = np.diff(off)[probe[:4, 0]]
	for j in range(4):
		assert (I3[j, :sizes[j]] >= 0).all() and (I3[j, sizes[j]:] == -1).all() and (D3[j, sizes[j]:] == np.finfo(np.float32).min).all()
	# determinism: the same seed builds the same index
	again = build_flat_or_ivff_index(X, force_exact_search=False)
	assert torch.equal(again.centroids, index.centroids) and torch.equal(again._ids, index._ids)


def test_ivf_bf16_lists_on_the_bf16_matrix_cores(gpu):
	"""An index built with dtype = "bf16" keeps a bf16 copy of its list-ordered vectors; the batched search scores it against bf16-rounded
	queries with one v_mfma_f32_32x32x16_bf16 GEMM per list (anncur_ivf_group_scores_dev, ANNCUR_BF16).  Same lists, same probes as the fp32 index;
	on inputs that ARE bf16 values the scores are the exact fp32-accumulated products: equal to the fp32 index's to round-off, same ids.
	Ragged sizes: d not a multiple of 32 (a partial k-tile), partial 64-tiles of pairs and of vectors, an empty list."""
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	g = np.random.default_rng(23)
	n, d, nq, k = 20000, 200, 1000, 20
	centers = g.standard_normal((40, d)).astype(np.float32) * 2
	X = torch.tensor(centers[g.integers(0, 40, n)] + g.standard_normal((n, d)).astype(np.float32)).bfloat16().float().numpy()
	q = torch.tensor(centers[g.integers(0, 40, nq)] + g.standard_normal((nq, d)).astype(np.float32)).bfloat16().float().numpy()
	a = IVFFlatIPIndex(d, 100, niter=4, dtype="fp32"); a.train(X); a.add(X); a.nprobe = 7
	b = IVFFlatIPIndex(d, 100, niter=4, dtype="bf16"); b.train(X); b.add(X); b.nprobe = 7
	assert torch.equal(a.centroids, b.centroids) and torch.equal(a._ids, b._ids) and b._Xs16 is not None and b._Xs16.dtype == torch.bfloat16
	Da, Ia = a.search(q, k)
	Db, Ib = b.search(q, k)
	np.testing.assert_allclose(Db, Da, rtol=2e-5, atol=2e-4)
	assert np.mean([len(set(x) & set(y)) / k for x, y in zip(Ia.tolist(), Ib.tolist())]) > 0.999
	np.testing.assert_allclose(Db, np.take_along_axis(q @ X.T, Ib, axis=1), rtol=2e-5, atol=2e-4)   # reported scores are the true inner products
	# below the batching threshold the per-query kernel runs on the fp32 lists: same answer
	Dc, Ic = b.search(q[:50], k)
	np.testing.assert_allclose(Dc, Db[:50], rtol=2e-5, atol=2e-4)
	# device-resident entry point: same results, tensors on the device
	v, i = b.search_device(torch.as_tensor(q).cuda(), k)
	assert v.is_cuda and i.is_cuda and np.array_equal(i.cpu().numpy().astype(np.int64), Ib)


def test_ivf_spherical_kmeans_keeps_lists_balanced_on_varying_norms(gpu):
	"""FAISS' IndexIVF trains its inner-product quantiser with cp.spherical = true: centroids are renormalised (fvec_renorm_L2) after
	every update.  With arg-max inner-product assignment an unnormalised mean of large-norm points keeps attracting points: on vectors
	whose norms vary by 10x the plain means give a few huge lists (scan cost = the probed lists' sizes) -- the spherical update (the
	default here) must keep the lists balanced, unit-norm, and at least as good in recall at the reference's nprobe."""
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	from anncur_amd import ops
	from oracle import cur_oracle as O
	g = np.random.default_rng(3)
	n, d, nq, k, nlist = 30000, 64, 400, 10, 173
	dirs = g.standard_normal((48, d)).astype(np.float32)
	X = dirs[g.integers(0, 48, n)] + 0.6 * g.standard_normal((n, d)).astype(np.float32)
	X = (X * np.exp(g.uniform(np.log(0.3), np.log(3.0), (n, 1)))).astype(np.float32)          # norms spread over a decade
	q = (dirs[g.integers(0, 48, nq)] + 0.6 * g.standard_normal((nq, d))).astype(np.float32)
	rD, rI = O.flat_ip_search(X, q, k)
	stats = {}
	for sph in (True, False):
		index = IVFFlatIPIndex(d, nlist, spherical=sph)
		index.train(X); index.add(X)
		index.nprobe = int(np.floor(np.sqrt(nlist)))
		sizes = np.diff(index._offsets.cpu().numpy())
		D, I = index.search(q, k)
		recall = np.mean([len(set(a) & set(b)) / k for a, b in zip(I.tolist(), rI.tolist())])
		probe = np.argsort(-(q @ index.centroids.cpu().numpy().T), axis=1)[:, :index.nprobe]
		stats[sph] = dict(max=int(sizes.max()), imbalance=float((sizes.astype(np.float64) ** 2).sum() * nlist / n ** 2), recall=float(recall),
						  scanned=float(sizes[probe].sum(axis=1).mean()), norms=index.centroids.norm(dim=1).cpu().numpy())
	sp, pl = stats[True], stats[False]
	np.testing.assert_allclose(sp["norms"], 1.0, rtol=1e-5)                 # unit-norm centroids
	assert sp["imbalance"] < pl["imbalance"] and sp["max"] < pl["max"], (sp, pl)   # FAISS' imbalance factor: sum n_l^2 * nlist / n^2 (1 = uniform)
	assert sp["imbalance"] < 3.0, sp
	assert sp["recall"] >= pl["recall"] - 0.02 and sp["recall"] > 0.8, (sp, pl)
	# the op itself: rows to unit norm in place, a zero row stays zero
	M = torch.tensor(g.standard_normal((5, 37)).astype(np.float32), device=gpu); M[2] = 0
	ref = M / M.norm(dim=1, keepdim=True).clamp_min(1e-30)
	ops.renorm_rows(M)
	torch.testing.assert_close(M[[0, 1, 3, 4]], ref[[0, 1, 3, 4]], rtol=1e-6, atol=1e-7)
	assert float(M[2].abs().max()) == 0.0


def test_ivf_batched_search_equals_the_per_query_scan(gpu):
	"""Many queries (the reference's hard-negative mining, utils/data_process.py:343-365): pairs (query, probed list) grouped by list,
	each list one fp32-MFMA GEMM (anncur_ivf_group_scores_dev, ANNCUR_F32), exact scan over the lists side by side, column -> id map.  Same probed
	lists, same exact fp32 inner products as the per-query kernel: same ids (boundary near-ties aside), scores equal to round-off;
	padding when k exceeds the probed lists; ragged lists incl. an empty one."""
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	g = np.random.default_rng(11)
	n, d, nq, k = 30000, 200, 1500, 20
	centers = g.standard_normal((40, d)).astype(np.float32) * 2
	X = (centers[g.integers(0, 40, n)] + g.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
	q = (centers[g.integers(0, 40, nq)] + g.standard_normal((nq, d)).astype(np.float32)).astype(np.float32)
	index = IVFFlatIPIndex(d, 120, niter=4)
	index.train(X); index.add(X)
	index.nprobe = 9
	index.batched_from = 10 ** 9
	D0, I0 = index.search(q, k)                       # per-query kernel
	index.batched_from = 1
	D1, I1 = index.search(q, k)                       # batched
	np.testing.assert_allclose(D1, D0, rtol=1e-5, atol=1e-4)
	assert np.mean([len(set(a) & set(b)) / k for a, b in zip(I0.tolist(), I1.tolist())]) > 0.9995
	np.testing.assert_allclose(D1, np.take_along_axis(q @ X.T, I1, axis=1), rtol=1e-5, atol=1e-4)
	assert (D1[:, :-1] >= D1[:, 1:]).all() and all(len(set(r.tolist())) == k for r in I1)
	# one probed list, k larger than it: FAISS-style (-FLT_MAX, -1) padding from the batched path too
	index.nprobe = 1
	D2, I2 = index.search(q[:300], 600)
	off = index._offsets.cpu().numpy()
	C = index.centroids.cpu().numpy()
	first = np.argmax(q[:300] @ C.T, axis=1)
	sizes = np.diff(off)[first]
	for j in range(0, 300, 23):
		m = min(int(sizes[j]), 600)
		assert (I2[j, :m] >= 0).all() and (I2[j, m:] == -1).all() and (D2[j, m:] == np.finfo(np.float32).min).all()


@pytest.mark.parametrize("dtype,d,nlist,nprobe,nq,k", [
	("fp32", 200, 120, 9, 1500, 20),      # 64 x 64 fp32 tiles on packed rows
	("bf16", 200, 100, 7, 1000, 20),      # rows padded to 256 elements: the persistent 128 x 128-tile kernel, two pairs of k-tiles per tile
	("bf16", 300, 57, 5, 777, 128),       # 384 elements: three pairs; the scan's largest k; nq not a multiple of 256
	("bf16", 64, 300, 40, 600, 64),       # 128 elements: ONE pair of k-tiles (first = last); many small lists, empty ones among them; rows shorter than k
	("bf16", 96, 8, 3, 5000, 10),         # few long lists: many tiles per list, more tiles than resident workgroups
	("fp32", 33, 64, 64, 300, 100),       # every list probed
])
def test_ivf_search_grouped_call_equals_the_round4_sequence(gpu, dtype, d, nlist, nprobe, nq, k):
	"""anncur_ivf_search_grouped (round 5: pairs grouped by list on the device, packed score rows, ragged scan, 128 x 128 bf16 tiles) against
	the sequence of calls it replaces (ops.ivf_scan_grouped: stable pair sort, [nq x nprobe x lmax] score matrix pre-filled with -inf,
	64 x 64 tiles): the same MFMA products accumulated in the same order along d -- scores BIT-EQUAL, ids equal (ties: both scans prefer
	the smaller column and the packed layout keeps the columns' order), (-inf, -1) padding where the probed lists hold fewer than k vectors."""
	from anncur_amd.nearest_nbr import IVFFlatIPIndex
	from anncur_amd import ops
	g = np.random.default_rng(1000 + d)
	n = 20000
	centers = g.standard_normal((30, d)).astype(np.float32) * 2
	X = (centers[g.integers(0, 30, n)] + g.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
	q = torch.tensor((centers[g.integers(0, 30, nq)] + g.standard_normal((nq, d)).astype(np.float32)).astype(np.float32), device=gpu)
	index = IVFFlatIPIndex(d, nlist, niter=3, dtype=dtype)
	index.train(X); index.add(X)
	index.nprobe = nprobe
	index.batched_from = 1
	assert index._dp % (128 if dtype == "bf16" else 16) == 0 and ops.ivf_search_grouped_ok(k, nlist)
	index.grouped_call = True
	v1, i1 = index.search_device(q, k)
	index.grouped_call = False
	v0, i0 = index.search_device(q, k)
	torch.cuda.synchronize()
	assert torch.equal(v1, v0)
	assert torch.equal(i1, i0)
	sizes = np.diff(index._offsets.cpu().numpy())
	probe = ops.score_topk_dense(q, index.centroids, min(nprobe, nlist)).indices.cpu().numpy()
	have = np.minimum(sizes[probe].sum(1), k)
	i1h = i1.cpu().numpy()
	assert all((i1h[j, :have[j]] >= 0).all() and (i1h[j, have[j]:] == -1).all() for j in range(nq))
	if nlist == 300: assert sizes.min() < 64   # (the many-small-lists case)


def test_ivf_search_grouped_direct_call_ragged_rows_and_bad_arguments(gpu):
	"""ops.ivf_search_grouped on hand-built lists: bf16 rows of 80 elements (not a multiple of 64: the 64 x 64 bf16 tiles on packed rows),
	probe entries of -1 (skipped), a query whose probed lists are all empty; against a dense fp32 product restricted to the probed lists.
	The ragged scan on its own; the entry's refusals."""
	from anncur_amd import ops, _lib
	g = np.random.default_rng(5)
	n, dp, nlist, nq, nprobe, k = 3000, 80, 40, 300, 6, 50
	sizes = g.multinomial(n, g.dirichlet(np.ones(nlist) * 0.5)).astype(np.int64)
	sizes[[3, 17]] += sizes[[4, 18]]; sizes[[4, 18]] = 0                                 # two empty lists
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
	ids = g.permutation(n).astype(np.int32)
	Xs = torch.tensor(g.standard_normal((n, dp)).astype(np.float32)).bfloat16()
	Qh = torch.tensor(g.standard_normal((nq, dp)).astype(np.float32)).bfloat16()
	probe = np.stack([g.choice(nlist, nprobe, replace=False) for _ in range(nq)]).astype(np.int32)
	probe[5, 2:] = -1
	probe[9, :] = [4, 18, -1, -1, -1, -1]                                                # nothing to scan
	got = ops.ivf_search_grouped(Xs.to(gpu), torch.tensor(off, device=gpu), torch.tensor(ids, device=gpu), sizes, Qh.to(gpu), torch.tensor(probe, device=gpu), k)
	S = Qh.float().numpy().astype(np.float64) @ Xs.float().numpy().astype(np.float64).T
	gv, gi = got.values.cpu().numpy(), got.indices.cpu().numpy()
	for j in range(nq):
		rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in probe[j] if l >= 0] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
		m = min(k, len(rows))
		order = rows[np.argsort(-S[j, rows], kind="stable")[:m]]
		np.testing.assert_allclose(gv[j, :m], S[j, order], rtol=1e-5, atol=1e-4)
		assert (gv[j, m:] == -np.inf).all() and (gi[j, m:] == -1).all()
		assert len(set(gi[j, :m].tolist()) ^ set(ids[order].tolist())) <= 2               # (a boundary near-tie may swap)
	# the ragged scan alone against torch.topk of every row's prefix
	A = torch.randn(37, 5000, device=gpu)
	rl = torch.tensor(g.integers(64, 5001, 37).astype(np.int32), device=gpu); rl[0] = 64; rl[1] = 5000
	rl[2] = 10; rl[3] = 0; rl[4] = 6000                            # shorter than k (padded), empty, beyond the matrix (clamped to its width)
	r = ops.rowwise_topk_ragged(A, rl, 64)
	for j in range(37):
		n = min(int(rl[j]), A.shape[1]); m = min(n, 64)
		w = torch.topk(A[j, :n], m)
		assert torch.equal(r.values[j, :m], w.values) and torch.equal(r.indices[j, :m].long(), w.indices)
		assert (r.values[j, m:] == -float("inf")).all() and (r.indices[j, m:] == -1).all()
	Ab = A.bfloat16()
	rb = ops.rowwise_topk_ragged(Ab, rl, 10)
	for j in range(37):
		n = min(int(rl[j]), A.shape[1]); m = min(n, 10)
		assert torch.equal(rb.values[j, :m], torch.topk(Ab[j, :n].float(), m).values)
	with pytest.raises(_lib.AnncurHipError):
		ops.rowwise_topk_ragged(A, rl, 129)
	assert not ops.ivf_search_grouped_ok(129, 100) and not ops.ivf_search_grouped_ok(10, 8193)
	with pytest.raises(ValueError):
		ops.ivf_search_grouped(Xs.to(gpu), torch.tensor(off, device=gpu), torch.tensor(ids, device=gpu), sizes, Qh.float().to(gpu), torch.tensor(probe, device=gpu), k)


# ------------------------------------------------------------------ row-sharded evaluation: 2 ranks sharing the one GPU, gloo
def _sharded_worker(rank, world, port, q):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	from anncur_amd import harness
	from anncur_amd.dist import ShardedScoreMatrix, shard_bounds
	torch.manual_seed(0)
	A = torch.randn(1000, 32) @ torch.randn(32, 5000) / (32 ** 0.5) + 0.1 * torch.randn(1000, 5000)
	s, e = shard_bounds(1000, rank, world)
	sm = ShardedScoreMatrix(A[s:e].cuda(), 1000)
	res = harness.run_approx_eval_w_seed_sharded(sm, 128, 64, 10, 100, seed=1)
	if rank == 0:
		single = harness.run_approx_eval_w_seed("cur", A.cuda(), 128, 64, 10, 100, seed=1)
		q.put({t: {m: (float(res[t][m]), float(single[t][m])) for m in res[t]} for t in res})
	else:
		assert res is None
		q.put(None)
	dist.destroy_process_group()


def test_row_sharded_entry_A_equals_single_process(gpu):
	import torch.multiprocessing as mp
	ctx = mp.get_context("spawn")
	q = ctx.Queue()
	port = 29700 + os.getpid() % 200
	procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
	for p in procs: p.start()
	outs = [q.get(timeout=300) for _ in procs]
	for p in procs: p.join(timeout=60)
	res = [o for o in outs if o is not None][0]
	for t in ("anchor", "non_anchor", "all"):
		for m, (sharded, single) in res[t].items():
			assert sharded == pytest.approx(single, rel=1e-5, abs=1e-6), (t, m)


# ------------------------------------------------------------------ bf16 entry A through anncur_eval_fused
def _bf16_cell_matrix():
	"""A bf16 score matrix large enough for the one-sweep route of a grid cell (cur.eval_rows / CURRowIndex.eval_cell -> ops.eval_fused)."""
	g = torch.Generator().manual_seed(21)
	Z = torch.randn(24, 20000, generator=g)
	A = torch.randn(1200, 24, generator=g) @ Z / (24 ** 0.5) + 0.1 * torch.randn(1200, 20000, generator=g)
	return A.bfloat16()


def _check_cell_against_oracle(got, want, top_k):
	"""recall statistics within 5e-3 (means) / one count (p50), error norms within 2e-3 relative -- the bf16 route's bar (bf16 copies of E and C_q)."""
	for t in ("anchor", "non_anchor", "all"):
		for m, w in want[t].items():
			g = float(got[t][m])
			if m.startswith("approx_error"):
				assert g == pytest.approx(float(w), rel=2e-3), (t, m, g, float(w))
			elif m.endswith("_p50"):
				assert abs(g - float(w)) <= (1.0 / top_k if "_frac_" in m else 1.0) + 1e-9, (t, m, g, float(w))
			elif m.endswith("_std"):
				assert abs(g - float(w)) <= (2e-2 if "_frac_" in m else 2e-2 * top_k), (t, m, g, float(w))
			else:
				assert abs(g - float(w)) <= (5e-3 if "_frac_" in m else 5e-3 * top_k), (t, m, g, float(w))


def test_entry_A_bf16_cell_through_eval_fused_matches_the_oracle(gpu):
	"""The product wiring of round 4's one-sweep route: harness.run_approx_eval_w_seed("cur") on a bf16 matrix (subset sums of the per-row error
	terms, square roots, the NaN of an empty subset) against the ORACLE's statement of crossenc.py:47-158 on the same bf16-rounded values
	(tie-stable loop: bf16 scores are tie-heavy and torch.topk's tie order is arbitrary)."""
	from anncur_amd import harness, ops
	from oracle import cur_oracle as O
	A = _bf16_cell_matrix()
	A_dev = A.to(gpu)
	top_k, k_retvr = 100, 100      # (top_k = k_retvr: recall well below 1, so the comparison has teeth)
	assert ops.eval_fused_ok(64, A_dev, 1200, 20000, k_retvr), "the cell must take the one-sweep route"
	taken = []
	orig = ops.eval_fused
	ops.eval_fused = lambda *a, **kw: (taken.append(1), orig(*a, **kw))[1]
	try:
		got = harness.run_approx_eval_w_seed("cur", A_dev, 128, 64, top_k, k_retvr, seed=3)
		full = harness.run_approx_eval_w_seed("cur", A_dev, 1200, 64, top_k, k_retvr, seed=3)     # every row an anchor: the non-anchor subset is empty
	finally:
		ops.eval_fused = orig
	assert len(taken) == 2, "harness.run_approx_eval_w_seed did not go through ops.eval_fused"
	want = O.run_approx_eval_w_seed("cur", A.float(), 128, 64, top_k, k_retvr, seed=3, stable=True)
	_check_cell_against_oracle(got, want, top_k)
	assert np.isnan(full["non_anchor"]["approx_error_relative"]) and float(full["non_anchor"]["approx_error"]) == 0.0   # 0 / 0, like torch.norm of an empty block
	assert float(full["anchor"]["approx_error"]) == pytest.approx(float(full["all"]["approx_error"]), rel=1e-6)


def _sharded_bf16_worker(rank, world, port, q):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	from anncur_amd import harness, ops
	from anncur_amd.dist import ShardedScoreMatrix, shard_bounds
	A = _bf16_cell_matrix()
	s, e = shard_bounds(1200, rank, world)
	A_loc = A[s:e].cuda()
	fused_ok = bool(ops.eval_fused_ok(64, A_loc, e - s, 20000, 100))
	sm = ShardedScoreMatrix(A_loc, 1200)
	res = harness.run_approx_eval_w_seed_sharded(sm, 128, 64, 100, 100, seed=3)
	q.put((rank, fused_ok, None if res is None else {t: {m: float(v) for m, v in d.items()} for t, d in res.items()}))
	dist.destroy_process_group()


def test_entry_A_bf16_cell_row_sharded_matches_the_oracle(gpu):
	"""The same cell on a row-sharded bf16 matrix (two ranks over gloo on the one GPU): CURRowIndex.eval_cell -> ops.eval_fused on every rank's
	block, the [counts, err, nrm] rows gathered to rank 0 -- against the oracle, to the same bar as the single-process cell."""
	import torch.multiprocessing as mp
	from oracle import cur_oracle as O
	ctx = mp.get_context("spawn")
	q = ctx.Queue()
	port = 29300 + os.getpid() % 200
	procs = [ctx.Process(target=_sharded_bf16_worker, args=(r, 2, port, q)) for r in range(2)]
	for p in procs: p.start()
	outs = [q.get(timeout=600) for _ in procs]
	for p in procs: p.join(timeout=60)
	assert all(ok for _, ok, _ in outs), "every rank's block must take the one-sweep route"
	res = [r for _, _, r in outs if r is not None]
	assert len(res) == 1
	want = O.run_approx_eval_w_seed("cur", _bf16_cell_matrix().float(), 128, 64, 100, 100, seed=3, stable=True)
	_check_cell_against_oracle(res[0], want, 100)


def test_entry_A_from_score_chunks_equals_combined_pickle(gpu, tmp_path):
	"""the producer's row chunks ingested straight to the device give the same results file as the combined pickle
	(the reference's pickle -> cat -> pickle -> load route), and the combiner writes that pickle with the reference's schema."""
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from eval import combine_chunked_computations as comb
	from anncur_amd import ingest
	from utils.zeshel_utils import N_ENTS_ZESHEL, score_matrix_filename
	torch.manual_seed(5)
	A = torch.randn(700, 24) @ torch.randn(24, 4000) / (24 ** 0.5) + 0.1 * torch.randn(700, 4000)
	res_dir = str(tmp_path / "res")
	files, start = [], 0
	for n in (300, 300, 100):
		path = ingest.chunk_filename(res_dir, "lego", n, N_ENTS_ZESHEL["lego"], mstart=start)
		_dump(path, A[start:start + n].clone(), test_data=[{"i": start + j} for j in range(n)])
		files.append(path); start += n
	common = ["--data_name", "lego", "--res_dir", res_dir, "--n_ment", "700", "--n_seeds", "2", "--disable_wandb", "1", "--eval_methods", "cur",
			  "--n_ment_anchors_vals", "100", "--n_ent_anchors_vals", "50", "--top_k_vals", "1,10", "--top_k_retr_vals", "100"]
	out_a = epA.main(common + ["--misc", "chunks", "--score_chunks"] + files)
	combined = comb.combine_m2e_eval_results(files, res_dir=res_dir, dataset_name="lego")
	assert combined == score_matrix_filename(res_dir, "lego", 700)
	out_b = epA.main(common + ["--misc", "pickle"])
	ra = json.load(open(os.path.join(out_a, "retrieval_wrt_exact_crossenc.json")))
	rb = json.load(open(os.path.join(out_b, "retrieval_wrt_exact_crossenc.json")))
	def same(a, b, path=""):
		if isinstance(a, dict):
			assert set(a) == set(b), path
			for key in a:
				same(a[key], b[key], path + "/" + key)
		elif "approx_error" in path:   # reduced with float atomics across column tiles: equal up to summation order
			assert a == pytest.approx(b, rel=1e-5), path
		else:                          # counts / recall statistics: identical
			assert a == b, path
	same(ra["cur"], rb["cur"])
	for bf in ("fp32", "bf16"):   # the device block equals the matrix (bf16: rounded once on the device)
		blk = ingest.load_score_chunks(files, gpu, bf)
		want = A.cuda() if bf == "fp32" else A.cuda().bfloat16()
		assert blk["A_local"].dtype == want.dtype and torch.equal(blk["A_local"], want) and blk["row_range"] == (0, 700)


def test_bench_contract_small_config(gpu):
	"""bench.py --full prints exactly one JSON line on stdout with the driver's keys plus `roofline` and `cpu_baseline` (small config)."""
	import subprocess, sys
	root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "small", "--steps", "3", "--warmup", "1", "--cpu-sample-queries", "256", "--full"],
						 capture_output=True, text=True, timeout=600)
	assert out.returncode == 0, out.stderr[-2000:]
	lines = [l for l in out.stdout.splitlines() if l.strip()]
	assert len(lines) == 1, out.stdout[-2000:]
	d = json.loads(lines[0])
	for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
				"roofline", "cpu_baseline"):
		assert key in d, key
	assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "queries/s" and d["scaling"] == "weak" and d["vs_baseline"] is None
	assert d["value"] > 0 and abs(d["value"] - 2000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
	assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and d["roofline"]["bound"] == "mfma"
	assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-9
	assert set(d["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"} and d["cpu_baseline"]["kind"] == "port"
	assert "workload" in d["config"] and "model" not in d["config"]
	# same queries through both paths: identical recall up to the tie-stable statement of the reference loop
	for key, want in d["cpu_baseline"]["recall_cpu_fp32_tie_stable"].items():
		assert abs(d["cpu_baseline"]["recall_gpu_same_queries"][key] - want) <= 5e-3, key


def test_entry_point_B_other_methods_match_reference_restatement(gpu, tmp_path):
	"""eval_method = fixed_anc_ent / fixed_anc_ent_cur (e2e pickle) and bienc (precomputed embeddings) through the CLI against a
	CPU restatement of the reference's lines (splits.py:305-358: the approximations; :399-429: the sweep via the oracle loop)."""
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	from oracle import cur_oracle as O
	g = torch.Generator().manual_seed(11)
	n_ent, n_train, n_test, r, n_fixed = 700, 50, 1200, 12, 40   # (1200 queries: one swapped boundary near-tie moves a mean by < 1e-3)
	Z = torch.randn(r, n_ent, generator=g)
	A_train = torch.randn(n_train, r, generator=g) @ Z / r ** 0.5 + 0.05 * torch.randn(n_train, n_ent, generator=g)
	A_test = torch.randn(n_test, r, generator=g) @ Z / r ** 0.5 + 0.05 * torch.randn(n_test, n_ent, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(n_train)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(n_train, n_train + n_test)))
	# entity-to-entity scores against 60 "fixed anchor" entities (same factor model), as the e2e dump holds them
	topk_ents = torch.randperm(n_ent, generator=g)[:60]
	e2e = (Z.t() @ Z[:, topk_ents]) / r + 0.02 * torch.randn(n_ent, 60, generator=g)          # n_ents x n_anchors
	with open(tmp_path / "e2e.pkl", "wb") as f:
		pickle.dump({"ent_to_ent_scores": e2e, "topk_ents": [topk_ents.numpy()]}, f)
	ment_emb = torch.randn(n_test, 32, generator=g); ent_emb = torch.randn(n_ent, 32, generator=g)
	np.save(tmp_path / "ment.npy", ment_emb.numpy()); np.save(tmp_path / "ent.npy", ent_emb.numpy())
	top_k, retr, ancs = [1, 10], [20, 50], [30, 45]
	common = ["--data_name", "lego", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"), "--train_data_file", str(tmp_path / "train.pkl"),
			  "--n_seeds", "1", "--top_k_vals", "1,10", "--top_k_retr_vals", "20,50", "--n_ent_anchors_vals", "30,45"]
	key = "exact_vs_reranked_approx_retvr~common_frac_mean"

	def sweep(approx_by_anchor):   # splits.py:399-429 with the oracle's statement of the per-query loop
		out = {}
		for n_anc, S in approx_by_anchor.items():
			for kr in retr:
				res = O.eval_approx_score_mat_for_all_topk(A_test, S, top_k, kr)
				for k, m in res.items():
					out[(k, kr, n_anc)] = m[key]
		return out

	def check(res_file, want, tol):
		with open(res_file) as f:
			got = json.load(f)["seed=0"]
		for (k, kr, n_anc), v in want.items():
			assert got[f"top_k={k}"][f"k_retvr={kr}"][f"anc_n_m={n_train}_anc_n_e={n_anc}"][key] == pytest.approx(v, abs=tol), (k, kr, n_anc)

	# fixed_anc_ent (splits.py:305-324): scores = A_test[:, first n fixed anchors] @ e2e[:, :n].T, the same result for every anchor count
	anc_ids = topk_ents[:n_fixed].numpy()
	S_fix = A_test[:, anc_ids] @ e2e[:, :n_fixed].t()
	f1 = epB.main(common + ["--eval_method", "fixed_anc_ent", "--e2e_fname", str(tmp_path / "e2e.pkl"), "--n_fixed_anc_ent", str(n_fixed), "--misc", "fae"])
	check(f1, sweep({a: S_fix for a in ancs}), 5e-3)
	# fixed_anc_ent_cur (splits.py:327-358): R = e2e[:, :n].T, anchors from rng(0) consumed over the anchor counts, U = pinv(R[:, anc])
	R = e2e[:, :n_fixed].t()
	rng = np.random.default_rng(seed=0)
	approx = {}
	for n_anc in ancs:
		anc = sorted(rng.choice(n_ent, size=n_anc, replace=False))
		U = torch.tensor(np.linalg.pinv(R[:, anc].numpy()))
		approx[n_anc] = A_test[:, anc] @ (U @ R)
	f2 = epB.main(common + ["--eval_method", "fixed_anc_ent_cur", "--e2e_fname", str(tmp_path / "e2e.pkl"), "--n_fixed_anc_ent", str(n_fixed), "--misc", "faec"])
	check(f2, sweep(approx), 5e-3)
	# bienc (splits.py:283): scores = mention_embeds @ label_embeds.T from precomputed embeddings
	f3 = epB.main(common + ["--eval_method", "bienc", "--mention_embeds_file", str(tmp_path / "ment.npy"), "--entity_embeds_file", str(tmp_path / "ent.npy"), "--misc", "bi"])
	check(f3, sweep({a: ment_emb @ ent_emb.t() for a in ancs}), 5e-3)


def test_entry_point_B_fixed_anc_ent_methods_match_reference_goldens(gpu, tmp_path, golden_dir, golden_meta):
	"""a13 against the REFERENCE: eval_method = fixed_anc_ent / fixed_anc_ent_cur through this build's CLI with the default
	(= the reference's hard-coded) grids, against what the reference's own run_eval_method returned on the same pickles
	(oracle/make_golden.py (viii): tests/golden/fixed_anc_ent_1100.npz, 4704 cells per method).  A cell may differ by two swapped boundary
	near-ties among its 150 queries (fp32 summation order); at least 97 % of the cells must agree to the reference's own 4 decimals."""
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	gold = np.load(os.path.join(golden_dir, "fixed_anc_ent_1100.npz"))
	g = torch.Generator().manual_seed(13)
	n_ent, n_train, n_test, r, n_fixed = 1100, 50, 150, 12, 40
	Z = torch.randn(r, n_ent, generator=g)
	A_train = torch.randn(n_train, r, generator=g) @ Z / r ** 0.5 + 0.05 * torch.randn(n_train, n_ent, generator=g)
	A_test = torch.randn(n_test, r, generator=g) @ Z / r ** 0.5 + 0.05 * torch.randn(n_test, n_ent, generator=g)
	topk_ents = torch.randperm(n_ent, generator=g)[:60]
	e2e = (Z.t() @ Z[:, topk_ents]) / r + 0.02 * torch.randn(n_ent, 60, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(n_train)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(n_train, n_train + n_test)))
	with open(tmp_path / "e2e.pkl", "wb") as f:
		pickle.dump({"ent_to_ent_scores": e2e, "topk_ents": [topk_ents.numpy()]}, f)
	common = ["--data_name", "lego", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"), "--train_data_file", str(tmp_path / "train.pkl"),
			  "--n_seeds", "1", "--e2e_fname", str(tmp_path / "e2e.pkl"), "--n_fixed_anc_ent", str(n_fixed), "--pinv", "numpy"]
	for method in ("fixed_anc_ent", "fixed_anc_ent_cur"):
		assert golden_meta["fixed_anc_ent"][method]["cells"] == len(gold[f"{method}_keys"]) == 4704
		res_file = epB.main(common + ["--eval_method", method, "--misc", method])
		with open(res_file) as f:
			got = json.load(f)["seed=0"]
		n_cells = n_exact = 0
		worst = 0.0
		for (tk, kr, na), want_cnt, want_frac in zip(gold[f"{method}_keys"].tolist(), gold[f"{method}_common_mean"].tolist(), gold[f"{method}_common_frac_mean"].tolist()):
			if method == "fixed_anc_ent_cur" and na == 0:
				continue   # zero anchors: S_hat = 0, every item ties, and the reference's own number is whatever order torch.topk returns
			cell = got[f"top_k={tk}"][f"k_retvr={kr}"][f"anc_n_m={n_train}_anc_n_e={na}"]
			d = abs(cell["exact_vs_reranked_approx_retvr~common_mean"] - want_cnt)
			assert d <= 2.0 / n_test + 1.01e-4, (method, tk, kr, na, cell["exact_vs_reranked_approx_retvr~common_mean"], want_cnt)
			assert abs(cell["exact_vs_reranked_approx_retvr~common_frac_mean"] - want_frac) <= 2.0 / n_test / tk + 1.01e-4, (method, tk, kr, na)
			n_cells += 1; n_exact += d <= 1.01e-4; worst = max(worst, d)
		assert n_cells >= 4500 and n_exact >= 0.97 * n_cells, (method, n_cells, n_exact, worst)
