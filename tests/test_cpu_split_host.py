"""Host side of the split-bf16 ("bf16x3") route: no GPU needed."""
import pytest
import torch


@pytest.mark.parametrize("K,Kp", [(85, 256), (86, 512), (170, 512), (171, 640), (256, 768), (768, 2304), (1366, None)])
def test_split_kp(K, Kp):
	from anncur_amd import ops
	assert ops.split_kp(K) == Kp
	assert Kp is None or (Kp >= 3 * K and Kp == ops.padded_k(3 * K))


def test_split_candidates():
	from anncur_amd import ops
	assert ops.split_candidates(100000, 100) == 100 + max(ops.SPLIT_RESCORE_EXTRA, 100 // 8)
	assert ops.split_candidates(100000, 1000) == 1000 + max(ops.SPLIT_RESCORE_EXTRA, 125)
	assert ops.split_candidates(100000, 2040) == ops._lib.MAX_TOPK and ops.split_candidates(50, 40) == 50
	assert ops.split_candidates(100000, 100, extra=0) == 100


def test_both_parsers_take_compute_dtype():
	from eval import run_retrieval_eval_wrt_exact_crossenc as epA
	from eval import run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits as epB
	a = epA.build_parser()
	assert a.parse_args(["--res_dir", "r"]).compute_dtype == "auto"
	assert a.parse_args(["--res_dir", "r", "--compute_dtype", "bf16x3"]).compute_dtype == "bf16x3"
	b = epB.build_parser()
	assert b.parse_args(["--res_dir", "r", "--test_data_file", "t"]).compute_dtype == "auto"
	assert b.parse_args(["--res_dir", "r", "--test_data_file", "t", "--compute_dtype", "bf16x3"]).compute_dtype == "bf16x3"
	for p, base in ((a, ["--res_dir", "r"]), (b, ["--res_dir", "r", "--test_data_file", "t"])):
		with pytest.raises(SystemExit):
			p.parse_args(base + ["--compute_dtype", "fp16"])


def test_unknown_compute_dtype_still_raises():
	from anncur_amd.cur import COMPUTE_DTYPES, CURApprox
	assert "bf16x3" in COMPUTE_DTYPES
	A = torch.arange(20, dtype=torch.float32).reshape(4, 5)
	with pytest.raises(ValueError, match="compute_dtype = nope not supported"):
		CURApprox(rows=A[[0, 2]], cols=A[:, [1, 3]], row_idxs=[0, 2], col_idxs=[1, 3], approx_preference="rows", compute_dtype="nope", device="cpu")


def test_ops_refuse_cpu_tensors():
	from anncur_amd import _lib, ops
	with pytest.raises(_lib.AnncurHipError):
		ops.pack_split_bf16(torch.zeros(2, 3), 0)
	with pytest.raises(_lib.AnncurHipError):
		ops.rescore_topk(torch.zeros(2, 3), torch.zeros(4, 3), torch.zeros(2, 2, dtype=torch.int32), 1)
