"""The table of tests/test_gpu_graph_replay.py cannot silently fall behind include/anncur_hip.h: every function the header declares with a
`void *stream` parameter is named by exactly one of the case table (a case declares the C symbols it issues) and the exclusion list (which
requires a reason).  Runs without a GPU: the table is plain data, nothing in it touches a device until a case runs."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_graph_replay as table  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_prototypes():
	"""name -> argument text of every function declared in the header (comments stripped, as tests/test_cpu_host.py reads it)."""
	src = open(os.path.join(ROOT, "include", "anncur_hip.h")).read()
	src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
	return dict(re.findall(r"\b(anncur_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))


def _stream_functions():
	return sorted(n for n, args in _header_prototypes().items() if re.search(r"\bvoid\s*\*\s*stream\b", args))


def test_the_parser_sees_the_header():
	protos = _header_prototypes()
	from anncur_amd import _lib
	assert sorted(protos) == sorted(_lib.SIGNATURES), "the prototype parser and the ctypes SIGNATURES disagree about the header"
	streams = _stream_functions()
	assert len(streams) >= 55 and "anncur_eval_topk" in streams and "anncur_svd_sweep" in streams
	for host_only in ("anncur_version", "anncur_score_topk_plan_ex", "anncur_lstsq_state_bytes", "anncur_ivf_search_tile"):
		assert host_only in protos and host_only not in streams


def test_every_stream_function_is_in_the_table_or_excluded_with_a_reason():
	streams = set(_stream_functions())
	in_cases = {}
	for c in table.CASES:
		assert c.symbols, f"case {c.name} declares no C symbol"
		for s in c.symbols:
			in_cases.setdefault(s, []).append(c.name)
	unknown = sorted((set(in_cases) | set(table.EXCLUDED)) - streams)
	assert not unknown, f"named in the table or the exclusion list, but not a `void *stream` function of the header: {unknown}"
	both = sorted(set(in_cases) & set(table.EXCLUDED))
	assert not both, f"both in a case and excluded: {both}"
	missing = sorted(streams - set(in_cases) - set(table.EXCLUDED))
	assert not missing, f"no graph-replay case and no exclusion for: {missing}"
	for name, reason in table.EXCLUDED.items():
		assert isinstance(reason, str) and len(reason.strip()) >= 20, f"{name}: an exclusion needs a reason"


def test_case_names_are_unique_and_cases_are_complete():
	names = [c.name for c in table.CASES]
	assert len(names) == len(set(names))
	for c in table.CASES:
		for attr in ("make", "load", "call", "check"):
			assert callable(getattr(c, attr)), (c.name, attr)


def test_the_check_fails_when_the_table_falls_behind(monkeypatch):
	"""Dropping a case, or a new `void *stream` function in the header, is seen."""
	import pytest
	victim = next(c for c in table.CASES if c.symbols == ("anncur_filter_topk",))
	monkeypatch.setattr(table, "CASES", [c for c in table.CASES if c.symbols != victim.symbols])
	with pytest.raises(AssertionError, match="anncur_filter_topk"):
		test_every_stream_function_is_in_the_table_or_excluded_with_a_reason()
	monkeypatch.undo()
	real = _header_prototypes()
	monkeypatch.setitem(globals(), "_header_prototypes", lambda: dict(real, anncur_new_call="const void *x, void *stream"))
	with pytest.raises(AssertionError, match="anncur_new_call"):
		test_every_stream_function_is_in_the_table_or_excluded_with_a_reason()
