#!/usr/bin/env python
"""Entry point B -- drop-in for the reference's eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py.

Same flags; reads the train/test split pickles (keys ment_to_ent_scores, mention_tokens_list, ment_idxs); writes
{res_dir}/method={eval_method}_{misc}.json with res["seed=s"]["top_k=.."]["k_retvr=.."]["anc_n_m=.._anc_n_e=.."][metric] and
res["other_args"]["retriever_params"], the layout eval/compile_emnlp_retrieval_eval_wrt_exact_crossenc.py:334 consumes.
Methods: cur and fixed_anc_ent_cur run fully on the GPU; bienc / tfidf / fixed_anc_ent run from PRECOMPUTED embeddings
(--mention_embeds_file / --entity_embeds_file, or the e2e pickle): the encoders themselves are out of scope.
"""
import argparse
import json
import logging
import os
import pickle
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

import numpy as np
import torch

from utils.zeshel_utils import get_dataset_info, get_zeshel_world_info

logging.basicConfig(stream=sys.stderr, format="%(asctime)s - %(levelname)s - %(name)s - %(message)s ",
					datefmt="%d/%m/%Y %H:%M:%S", level=logging.INFO)
LOGGER = logging.getLogger(__name__)


def _ints(s):
	return [int(x) for x in s.split(",") if x != ""]


def _rounds(s):
	n = int(s)
	if n < 1:
		raise argparse.ArgumentTypeError("--adaptive_rounds needs an integer >= 1")
	return n


def _temperature(s):
	t = float(s)
	if not (t > 0 and t < float("inf")):
		raise argparse.ArgumentTypeError("--adaptive_temperature needs a finite number > 0")
	return t


def _seed(s):
	n = int(s)
	if not 0 <= n < 1 << 64:
		raise argparse.ArgumentTypeError("--adaptive_seed needs an integer in [0, 2^64)")
	return n


def _rcond(s):
	r = float(s)
	if not (0.0 <= r < 1.0):
		raise argparse.ArgumentTypeError("--pinv_rcond needs a number in [0, 1)")
	return r


def run_eval_method(curr_method, test_data_file, train_data_file, args, seed, device):
	from anncur_amd import harness, ops
	LOGGER.info("Loading precomputed ment_to_ent scores")
	test = harness.load_score_pickle(test_data_file)
	A_test = test["ment_to_ent_scores"]
	test_ment_idxs = test["ment_idxs"]  # required by the reference as well (splits.py:225)
	n_test, n_ent = A_test.shape
	train = harness.load_score_pickle(train_data_file)
	A_train = train["ment_to_ent_scores"]
	n_train, n_ent_train = A_train.shape
	assert n_ent_train == n_ent, "Train and test entities differ! Use entity_id_list from data dump to resolve this"
	grids = harness.default_grids_B(n_ent, curr_method)
	for key in ("top_k_vals", "top_k_retr_vals", "n_ent_anchors_vals"):
		if getattr(args, key) is not None:
			grids[key] = sorted(set(getattr(args, key)))
	A_test_dev = harness.to_device_matrix(A_test, device, args.dtype)
	pool_kw = {} if args.rerank_pool == "retrieved" else {"rerank_pool": args.rerank_pool}   # (non-CUR methods ignore the flag)
	if args.adaptive_rounds >= 2 and curr_method == "cur":
		pool_kw = dict(pool_kw, adaptive_rounds=args.adaptive_rounds)   # (1 = today's call; the other methods ignore the flag)
		if args.adaptive_incremental:
			pool_kw = dict(pool_kw, adaptive_incremental=True)
		if args.adaptive_strategy != "topk":
			pool_kw = dict(pool_kw, adaptive_strategy=args.adaptive_strategy)
		if args.adaptive_temperature != 1.0:
			pool_kw = dict(pool_kw, adaptive_temperature=args.adaptive_temperature)
		if args.adaptive_seed != 0:
			pool_kw = dict(pool_kw, adaptive_seed=args.adaptive_seed)
	if args.anchor_selection != "random" and curr_method == "cur":
		pool_kw = dict(pool_kw, anchor_selection=args.anchor_selection)   # (random = today's call; the other methods ignore the flag)
	if args.pinv_rcond is not None and curr_method == "cur":
		pool_kw = dict(pool_kw, pinv_rcond=args.pinv_rcond)   # (None = today's call; the other methods build no pseudo-inverse through --pinv)
	if args.rank_metrics and curr_method == "cur":
		pool_kw = dict(pool_kw, rank_metrics=True)   # (off = today's call; the other methods ignore the flag)
	LOGGER.info(f"Computing approximate test mention-to-entity scores using method={curr_method}")
	if curr_method == "cur":
		A_train_dev = harness.to_device_matrix(A_train, device, args.dtype)
		res = harness.run_eval_method_cur(A_test_dev, A_train_dev, seed, grids, compute_dtype=None if args.compute_dtype == "auto" else args.compute_dtype,
										  progress=lambda j, n: LOGGER.info(f"anchor count {j + 1}/{n}"), pinv_backend=args.pinv, **pool_kw)
	elif curr_method in ("bienc", "tfidf"):
		if not (args.mention_embeds_file and args.entity_embeds_file):
			raise SystemExit(f"eval_method={curr_method}: pass --mention_embeds_file and --entity_embeds_file (.npy, or .npz as scipy.sparse.save_npz "
							 "writes a CSR matrix); computing them needs the reference's encoders, which are out of scope of this build")
		ment, ent = harness.load_embeds(args.mention_embeds_file), harness.load_embeds(args.entity_embeds_file)
		if curr_method == "tfidf" and (ment.n_rows if isinstance(ment, ops.SparseCSR) else ment.shape[0]) != n_test:
			ment = harness.take_embed_rows(ment, test_ment_idxs)        # splits.py:378
		# a sparse side stays sparse (harness.run_eval_method_embeds retrieves through the term-major index; a dense other side is sparsified there)
		ment, ent = (e if isinstance(e, ops.SparseCSR) else torch.as_tensor(e, dtype=torch.float32).to(device) for e in (ment, ent))
		res = harness.run_eval_method_embeds(A_test_dev, ment, ent, n_train, grids)
	elif curr_method in ("fixed_anc_ent", "fixed_anc_ent_cur"):
		if not os.path.isfile(args.e2e_fname):
			raise SystemExit(f"File {args.e2e_fname} not found")
		with open(args.e2e_fname, "rb") as fin:
			e2e = pickle.load(fin)
		full = torch.as_tensor(np.asarray(e2e["ent_to_ent_scores"]), dtype=torch.float32).to(device)   # n_ents x n_anchors
		if curr_method == "fixed_anc_ent":
			anc = [int(x) for x in np.asarray(e2e["topk_ents"][0])[:args.n_fixed_anc_ent]]
			ment = ops.gather_cols(A_test_dev, anc, out_dtype=torch.float32)
			res = harness.run_eval_method_embeds(A_test_dev, ment, full[:, :args.n_fixed_anc_ent].contiguous(), n_train, grids)
		else:
			res = harness.run_eval_method_fixed_anc_ent_cur(A_test_dev, full, args.n_fixed_anc_ent, grids, key_n_m=n_train,
															**({} if args.rerank_pool == "retrieved" else {"rerank_pool": args.rerank_pool}))
	else:
		raise NotImplementedError(f"Method = {curr_method} not supported")
	params = {"top_k_retr_vals": grids["top_k_retr_vals"], "top_k_vals": grids["top_k_vals"], "n_ent_anchors_vals": grids["n_ent_anchors_vals"]}
	return res, params


def run(args, device):
	eval_method, n_seeds = args.eval_method, args.n_seeds
	if device.type == "cuda":
		torch.cuda.set_device(device)   # the launch stream and torch's allocations follow --device
	assert eval_method == "cur" or n_seeds == 1, f"n_seed = {n_seeds} only allowed for eval_method = cur "
	if args.use_wandb:
		LOGGER.info("--use_wandb: wandb logging is optional and not configured in this build; continuing without it")
	eval_res, retvr_params = {}, {}
	for seed in range(n_seeds):
		curr_res, retvr_params = run_eval_method(eval_method, args.test_data_file, args.train_data_file, args, seed, device)
		eval_res[f"seed={seed}"] = curr_res
	arg_dict = dict(args.__dict__)
	if args.rerank_pool == "retrieved":
		del arg_dict["rerank_pool"]   # the default run writes the output it wrote before the flag existed, byte for byte
	if args.adaptive_rounds == 1:
		del arg_dict["adaptive_rounds"]   # (the same rule)
	if not args.adaptive_incremental:
		del arg_dict["adaptive_incremental"]   # (the same rule)
	if not args.rank_metrics:
		del arg_dict["rank_metrics"]   # (the same rule)
	for key, default in (("adaptive_strategy", "topk"), ("adaptive_temperature", 1.0), ("adaptive_seed", 0), ("anchor_selection", "random"), ("pinv_rcond", None)):
		if getattr(args, key) == default:
			del arg_dict[key]   # (the same rule)
	eval_res["other_args"] = arg_dict
	eval_res["other_args"]["retriever_params"] = retvr_params
	res_file = f"{args.res_dir}/method={eval_method}_{args.misc}.json"
	Path(os.path.dirname(res_file)).mkdir(exist_ok=True, parents=True)
	with open(res_file, "w") as fout:
		json.dump(eval_res, fout, indent=4)
	LOGGER.info(f"Wrote {res_file}")
	return res_file


class _Parser(argparse.ArgumentParser):
	"""argparse with the rules that span two flags: a deterministic anchor selection has no seeds to average over, and only a backend that
	can truncate takes --pinv_rcond."""

	def parse_args(self, args=None, namespace=None):
		ns = super().parse_args(args, namespace)
		if ns.anchor_selection == "pivoted" and ns.n_seeds > 1:
			self.error(f"--anchor_selection pivoted is deterministic: --n_seeds {ns.n_seeds} would repeat one result (use --n_seeds 1)")
		if ns.pinv_rcond is not None and ns.pinv not in ("svd", "numpy"):
			self.error(f"--pinv_rcond needs --pinv svd or numpy: Newton-Schulz (--pinv {ns.pinv}) cannot truncate")
		if ns.rank_metrics and ns.adaptive_rounds != 1:
			self.error(f"--rank_metrics needs --adaptive_rounds 1: the pool of --adaptive_rounds {ns.adaptive_rounds} is no prefix of one ranking")
		return ns


def build_parser(worlds=None):
	worlds = get_zeshel_world_info() if worlds is None else worlds
	parser = _Parser(description="Run eval for various retrieval methods wrt exact crossencoder scores using a fixed train/test "
												 "split. This evaluation does not use ground-truth entity information into account")
	parser.add_argument("--data_name", type=str, choices=[w for _, w in worlds], help="Dataset name")
	parser.add_argument("--eval_method", type=str, choices=["cur", "bienc", "fixed_anc_ent", "fixed_anc_ent_cur", "tfidf"], help="Eval method")
	parser.add_argument("--res_dir", type=str, required=True, help="Result directory")
	parser.add_argument("--test_data_file", type=str, required=True, help="Test data file")
	parser.add_argument("--train_data_file", type=str, default="", help="Training data file. Used for method=cur")
	parser.add_argument("--n_seeds", type=int, default=1, help="Number of seeds to run")
	parser.add_argument("--bi_model_file", type=str, default="", help="File for biencoder ckpt (not used: pass precomputed embeddings instead)")
	parser.add_argument("--batch_size", type=int, default=50, help="Batch size to use with biencoder (unused)")
	parser.add_argument("--e2e_fname", type=str, default="", help="File w/ entity2entity scores. Used for method=fixed_anc_ent(_cur)")
	parser.add_argument("--n_fixed_anc_ent", type=int, default=0, help="Number of fixed anchor entities to use")
	parser.add_argument("--mention_file", type=str, default="", help="Raw mention data (tfidf; unused: pass precomputed embeddings)")
	parser.add_argument("--entity_file", type=str, default="", help="Raw entity data (tfidf; unused: pass precomputed embeddings)")
	parser.add_argument("--mode", type=str, choices=["eval", "plot", "eval_n_plot"], default="eval", help="To run in eval mode or just plotting or both")
	parser.add_argument("--misc", type=str, default="", help="Misc suffix")
	parser.add_argument("--use_wandb", type=int, default=0, choices=[0, 1], help="1 to enable wandb and 0 to disable it ")
	# additions: grid overrides (defaults = the reference's hard-coded grids, splits.py:238-251), precomputed embeddings, device/dtype
	parser.add_argument("--top_k_vals", type=_ints, default=None)
	parser.add_argument("--top_k_retr_vals", type=_ints, default=None)
	parser.add_argument("--n_ent_anchors_vals", type=_ints, default=None)
	parser.add_argument("--mention_embeds_file", type=str, default="")
	parser.add_argument("--entity_embeds_file", type=str, default="")
	parser.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16"])
	parser.add_argument("--device", type=str, default="cuda:0")
	parser.add_argument("--pinv", type=str, default="auto", choices=["numpy", "device", "auto", "device32", "svd"],
						help="pseudo-inverse: numpy = the reference's numpy.linalg.pinv on the host (bit-identical U); device = fp64 Newton-Schulz on the GPU "
							 "(exact pseudo-inverse of the fp32 block, rounded once); auto = device while the block is well conditioned, else numpy; svd = Jacobi SVD in "
							 "fp64 on the GPU, truncated at --pinv_rcond (blocks up to 2048 on the short side and 8192 on the long one: cur_oracle only on small matrices)")
	parser.add_argument("--pinv_rcond", type=_rcond, default=None,
						help="with --pinv svd or numpy: singular values of the anchor block at or below this fraction of the largest are left out of the pseudo-inverse "
							 "(in [0, 1); default: the reference's 1e-15).  Newton-Schulz (auto, device, device32) cannot truncate: an error beside those")
	parser.add_argument("--rerank_pool", type=str, default="retrieved", choices=["retrieved", "retrieved+anchors"],
						help="items the exact re-rank of a CUR cell chooses from: retrieved = the k_retvr retrieved items (the reference's cell); retrieved+anchors = "
							 "additionally report, under exact_vs_reranked_approx_retvr_w_anchors~..., the pool of the anchor items (whose exact scores every query has "
							 "paid for) plus k_retvr NEW items, a budget of n_anc + k_retvr exact scores per query (cur, fixed_anc_ent_cur; other methods ignore it)")
	parser.add_argument("--adaptive_rounds", type=_rounds, default=1,
						help="N >= 2 (eval_method cur): every cell with k_retvr divisible by N additionally reports, under exact_vs_reranked_adaptive_retvr~..., the pool "
							 "of the adaptive multi-round search -- the anchor items plus N rounds of k_retvr / N new items, each round's weights solved per query from "
							 "everything scored so far -- at the same budget of n_anc + k_retvr exact scores per query; 1 (default) = today's run and output")
	parser.add_argument("--adaptive_incremental", action="store_true",
						help="with --adaptive_rounds N >= 2: extend each query's Cholesky factorisation round by round instead of solving from scratch (the same "
							 "output keys; needs n_anc + (N - 1) k_retvr / N <= the number of training queries, cells beyond that are left out and logged); "
							 "without --adaptive_rounds N >= 2, and for the other methods, it has no effect")
	parser.add_argument("--adaptive_strategy", type=str, default="topk", choices=["topk", "softmax"],
						help="with --adaptive_rounds N >= 2: how a round picks its new items: topk = the k_retvr / N best of the round's approximate scores (today's run "
							 "and output); softmax = that many items drawn without replacement with probability proportional to softmax(scores / temperature), every "
							 "round, reported under exact_vs_reranked_adaptive_softmax_retvr~... instead; without --adaptive_rounds N >= 2 it has no effect")
	parser.add_argument("--adaptive_temperature", type=_temperature, default=1.0, help="temperature of --adaptive_strategy softmax (finite, > 0; default 1)")
	parser.add_argument("--adaptive_seed", type=_seed, default=0,
						help="seed of --adaptive_strategy softmax's noise, in [0, 2^64) (default 0); round r draws from stream r, a query from its row number")
	parser.add_argument("--anchor_selection", type=str, default="random", choices=["random", "pivoted"],
						help="eval_method cur: how the index picks its anchor items: random = sorted(rng.choice(...)) per anchor count and seed (the reference's choice; "
							 "today's run and output); pivoted = the sorted first n_anc items of one column-pivoted QR selection from the training matrix, on the "
							 "device (deterministic: needs --n_seeds 1; anchor counts above the number of training queries, ANNCUR_MAX_TOPK or the numerical rank "
							 "are left out and logged)")
	parser.add_argument("--rank_metrics", action="store_true",
						help="eval_method cur with --adaptive_rounds 1: every top_k additionally reports, under res[seed][top_k=k][approx_rank][anc_n_m=.._anc_n_e=..], the "
							 "approximate rank of the exact top-k items over all (query, item) pairs -- exact_topk_approx_rank~mean / p50 / p90 / p99 / max -- and "
							 "k_retvr_for_recall~r, the smallest k_retvr whose retrieved lists hold the fraction r of them: the whole recall curve from one rank call "
							 "per anchor count, not limited to ANNCUR_MAX_TOPK; off (default) = today's run and output")
	parser.add_argument("--compute_dtype", type=str, default="auto", choices=["auto", "fp32", "bf16", "bf16x3"],
						help="arithmetic of the CUR retrieval: auto = by --dtype (fp32 matrix -> dense fp32 route, bf16 -> fused bf16 kernel); bf16x3 = for --dtype fp32: "
							 "operands split into bf16 hi + lo parts on the fused kernel, candidates rescored in fp32 (the fp32 route's values, S_hat never written)")
	return parser


def main(argv=None):
	worlds = get_zeshel_world_info()
	args = build_parser(worlds).parse_args(argv)
	_ = get_dataset_info(data_dir="../../data/zeshel", res_dir=args.res_dir, worlds=worlds)  # kept for parity with the reference's main()
	LOGGER.info(f"Running inference for world = {args.data_name}")
	return run(args, torch.device(args.device))


if __name__ == "__main__":
	main()
