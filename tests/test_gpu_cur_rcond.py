"""pinv_backend="svd" and rcond= through CURRowIndex and entry point B.

The data: a rank-32 + 0.05-noise score matrix with 3000 items; 96 anchor items; 96 anchor queries make the anchor block square and
ill-conditioned (cond_2 ~ 1e4: numpy.linalg.pinv at its rcond = 1e-15 inverts ~30 singular values that are noise), 192 make it healthy
(cond_2 ~ 160).  Reference figures, numpy fp64 alone, seeds 0 / 1 / 2: recall@10 at k_retvr = 100 is 0.5531 / 0.5594 / 0.4891 at rcond = 1e-15
and 1.0000 at rcond = 1e-2, which keeps 65 / 65 / 66 singular values.

The bound that holds the two backends together (test_backends_agree_on_U_within_the_fp64_bound) allows one fp32 rounding (2^-24) next to an
fp64-sized term, so it needs a reference that is good to fp64: backend "numpy" with a GIVEN rcond runs LAPACK in fp64 on the fp32 values and
rounds once (cur._pinv_host; without rcond it stays the reference's own fp32 call, bit for bit).  numpy's fp32 call could not serve: on the
host it is 1.35e-7 / 9.1e-8 / 9.4e-8 away from its own fp64 call at rcond = 1e-2 (seeds 0 / 1 / 2), the bound being 2.97e-8 / 3.21e-8 /
3.00e-8, and "svd" measured 1.49e-7 / 8.9e-8 / 8.9e-8 against it on an MI355X.  Against the fp64 call "svd" measured 0 (the same fp32 bits)
after the common rounding, 1.49e-8 / 1.98e-8 / 1.69e-8 (half an fp32 ulp of the entries) before it.  Needs an MI355X."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32.0            # tests/test_gpu_svd.py: 8 x the largest measured error ratio of the decomposition, rounded up to a power of two
EPS = 2.0 ** -53
SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def gpu():
	if not torch.cuda.is_available():
		pytest.skip("no GPU")
	return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def data(seed, n_train=96):
	"""(A_train fp32 [n_train x 3000], A_test fp32 [64 x 3000], 96 sorted anchor items): one generator, drawn in this order."""
	g = np.random.default_rng(seed)
	Z = g.standard_normal((32, 3000))
	A_train = (g.standard_normal((n_train, 32)) @ Z / np.sqrt(32) + 0.05 * g.standard_normal((n_train, 3000))).astype(np.float32)
	A_test = (g.standard_normal((64, 32)) @ Z / np.sqrt(32) + 0.05 * g.standard_normal((64, 3000))).astype(np.float32)
	anc = np.sort(g.choice(3000, 96, replace=False))
	for a in (A_train, A_test, anc):
		a.setflags(write=False)
	return A_train, A_test, anc


@functools.lru_cache(maxsize=None)
def built(seed, backend, rcond, n_train=96):
	"""(index, retrieved ids [64 x 100] on the host): one index per (seed, backend, rcond), shared by the tests."""
	from anncur_amd.cur import CURRowIndex
	A_train, A_test, anc = data(seed, n_train)
	index = CURRowIndex(torch.tensor(A_train).cuda(), anc.copy(), compute_dtype="fp32", pinv_backend=backend, rcond=rcond)
	ids = index.topk(torch.tensor(A_test[:, anc]).cuda(), 100).indices.cpu().numpy()
	return index, ids


def recall_at_10(seed, ids):
	A_test = data(seed)[1]
	exact = np.argsort(-A_test, axis=1, kind="stable")[:, :10]
	return float(np.mean([len(set(exact[q]) & set(ids[q])) / 10.0 for q in range(A_test.shape[0])]))


def block_svd(seed, n_train=96):
	A_train, _, anc = data(seed, n_train)
	return np.linalg.svd(A_train[:, anc].astype(np.float64), compute_uv=False)


def u_bound(U_ref, s, rank):
	xm = np.abs(U_ref).max()
	return C * 96 * EPS * (s[0] / s[rank - 1]) * xm + 2.0 ** -24 * xm


# ------------------------------------------------------------------ 6. parity on a healthy block
@pytest.mark.parametrize("seed", SEEDS)
def test_svd_without_rcond_matches_numpy_on_the_healthy_block(gpu, seed):
	a, _ = built(seed, "svd", None, 192)
	b, _ = built(seed, "numpy", None, 192)
	Ua, Ub = a.U.cpu().numpy().astype(np.float64), b.U.cpu().numpy().astype(np.float64)
	rel = np.abs(Ua - Ub).max() / np.abs(Ub).max()
	print(f"seed {seed}: 192 x 96 block, max|U_svd - U_numpy| / max|U_numpy| = {rel:.3e}")
	assert rel <= 1e-5
	assert a.rank == 96 and b.rank is None and b.singular_values is None
	s = block_svd(seed, 192)
	assert np.abs(a.singular_values.cpu().numpy() - s).max() <= C * 96 * EPS * s[0]


# ------------------------------------------------------------------ 7. the point of the feature
@pytest.mark.parametrize("seed", SEEDS)
def test_truncation_restores_recall_on_the_square_block(gpu, seed):
	s = block_svd(seed)
	assert np.abs(s / (1e-2 * s[0]) - 1.0).min() > 1e-6            # (the reference side: no singular value sits on the cutoff)
	index, ids = built(seed, "svd", 1e-2)
	_, ids_ref = built(seed, "numpy", None)
	r_svd, r_ref = recall_at_10(seed, ids), recall_at_10(seed, ids_ref)
	print(f"seed {seed}: recall@10 at k_retvr = 100: svd rcond 1e-2 {r_svd:.4f}, numpy rcond 1e-15 {r_ref:.4f}, rank {index.rank} of 96")
	assert r_svd >= 0.99
	assert r_svd - r_ref >= 0.3
	assert index.rank == int((s > 1e-2 * s[0]).sum())
	sv = index.singular_values.cpu().numpy()
	assert sv.dtype == np.float64 and sv.shape == (96,) and np.all(sv[:-1] >= sv[1:])
	assert np.abs(sv - s).max() <= C * 96 * EPS * s[0]


# ------------------------------------------------------------------ 8. backend agreement at the same rcond
@pytest.mark.parametrize("seed", SEEDS)
def test_backends_agree_on_the_retrieved_sets(gpu, seed):
	_, ids = built(seed, "svd", 1e-2)
	_, ids_np = built(seed, "numpy", 1e-2)
	assert all(set(ids[q]) == set(ids_np[q]) for q in range(ids.shape[0]))


@pytest.mark.parametrize("seed", SEEDS)
def test_svd_matches_the_fp64_pseudo_inverse_within_the_bound(gpu, seed):
	"""The new route against numpy.linalg.pinv in fp64 on the same fp32 values, same rcond: the bound of the truncation test."""
	A_train, _, anc = data(seed)
	index, _ = built(seed, "svd", 1e-2)
	s = block_svd(seed)
	U_ref = np.linalg.pinv(A_train[:, anc].astype(np.float64), rcond=1e-2)
	err, bound = np.abs(index.U.cpu().numpy().astype(np.float64) - U_ref).max(), u_bound(U_ref, s, index.rank)
	print(f"seed {seed}: max|U_svd - U_fp64| = {err:.3e}, bound {bound:.3e}")
	assert err <= bound


@pytest.mark.parametrize("seed", SEEDS)
def test_backends_agree_on_U_within_the_fp64_bound(gpu, seed):
	"""The two backends at the same rcond, held to the bound of the truncation test (tests/test_gpu_svd.py) with numpy's U as the reference."""
	a, _ = built(seed, "svd", 1e-2)
	b, _ = built(seed, "numpy", 1e-2)
	s = block_svd(seed)
	U_ref = b.U.cpu().numpy().astype(np.float64)
	err, bound = np.abs(a.U.cpu().numpy().astype(np.float64) - U_ref).max(), u_bound(U_ref, s, a.rank)
	print(f"seed {seed}: max|U_svd - U_numpy| = {err:.3e}, bound {bound:.3e}")
	assert err <= bound


# ------------------------------------------------------------------ 9. entry point B
def _dump(path, scores, **extra):
	os.makedirs(os.path.dirname(path), exist_ok=True)
	d = {"ment_to_ent_scores": scores, "ment_to_ent_scores.shape": tuple(scores.shape), "test_data": [], "mention_tokens_list": [[0] * 4] * scores.shape[0],
		 "entity_id_list": np.arange(scores.shape[1]), "entity_tokens_list": [], "arg_dict": {}}
	d.update(extra)
	with open(path, "wb") as f:
		pickle.dump(d, f)


def test_entry_point_B_with_svd_and_rcond(gpu, tmp_path):
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	g = torch.Generator().manual_seed(3)
	Z = torch.randn(16, 600, generator=g)
	A_train = torch.randn(60, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(60, 600, generator=g)
	A_test = torch.randn(40, 16, generator=g) @ Z / 4 + 0.05 * torch.randn(40, 600, generator=g)
	_dump(str(tmp_path / "train.pkl"), A_train, ment_idxs=list(range(60)))
	_dump(str(tmp_path / "test.pkl"), A_test, ment_idxs=list(range(60, 100)))
	common = ["--data_name", "lego", "--eval_method", "cur", "--res_dir", str(tmp_path / "out"), "--test_data_file", str(tmp_path / "test.pkl"),
			  "--train_data_file", str(tmp_path / "train.pkl"), "--top_k_vals", "1,10", "--top_k_retr_vals", "10,50", "--n_ent_anchors_vals", "20,60"]
	with open(epB.main(common + ["--misc", "svd", "--pinv", "svd", "--pinv_rcond", "0.01"])) as f:
		on = json.load(f)
	with open(epB.main(common + ["--misc", "dflt"])) as f:
		off = json.load(f)
	assert on["other_args"]["pinv"] == "svd" and on["other_args"]["pinv_rcond"] == 0.01
	assert off["other_args"]["pinv"] == "auto" and "pinv_rcond" not in off["other_args"]
	assert {k: v for k, v in on["other_args"].items() if k not in ("pinv", "pinv_rcond", "misc")} == {k: v for k, v in off["other_args"].items() if k not in ("pinv", "misc")}
	# the same cells, the rectangular 60 x 20 block and the square 60 x 60 one, with finite metrics
	cells_on, cells_off = on["seed=0"]["top_k=10"]["k_retvr=50"], off["seed=0"]["top_k=10"]["k_retvr=50"]
	assert set(cells_on) == set(cells_off) == {"anc_n_m=60_anc_n_e=20", "anc_n_m=60_anc_n_e=60"}
	for cell in cells_on.values():
		assert set(cell) == set(cells_off["anc_n_m=60_anc_n_e=20"]) and all(np.isfinite(v) for v in cell.values())
