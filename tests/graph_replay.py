"""The stream contract of include/anncur_hip.h, lines 12-14, as one procedure (no tests here; tests/fused_exact_cases.py is the precedent):
every call is asynchronous on the caller's stream, allocates nothing, never synchronises with the host and can be captured into a HIP graph.

run(case) captures the case's calls ONCE and replays the graph on OTHER data in the SAME buffers, with every output filled with 0xA5 bytes and
every workspace with 0xFF bytes first.  That is a deterministic test of four kinds of mistake an eager call on fresh inputs cannot show:
  - a launch, memset or copy on the NULL stream instead of `stream`: it is missing from the graph, the replay leaves poison (or stale data);
  - a value looked at on the host at call time and baked into a launch parameter: right for the captured data, wrong for the replayed data;
  - a workspace word the call expects to be zero, or left over from its own last run: the 0xFF poison breaks it;
  - a hidden allocation or synchronisation: the capture itself fails.

A case is an object with
  name, symbols   the id of the case and the C entry points (with a `void *stream`) it issues;
  make(seed)      host data, integer-valued where the operation allows it, so that the results are exact; seed 0 is data set A, 1 is B;
  load(data, bufs)  writes the data into the fixed device buffers of the dict `bufs` in place (put() allocates a buffer on its first use);
  call(bufs)      issues the call or calls on the current stream and returns the output tensors (fresh ones or buffers of `bufs`);
  check(data, outs) holds the eager outputs (host clones) against the host reference of the operation;
  workspaces(bufs)  the scratch buffers that need no pre-filling (default: every buffer whose name starts with "ws");
  canon(outs)     optional: the outputs in the form that is compared (ids sorted inside score ties where the operation leaves their order open);
  differ          optional: indices of the outputs that must differ between A and B (default: all of them)."""
import torch

OUT_POISON, WS_POISON = 0xA5, 0xFF


def put(bufs, name, host, device="cuda"):
	"""bufs[name] <- host tensor, in place: the buffer is allocated by the first call and keeps its address, shape and dtype afterwards."""
	host = host if torch.is_tensor(host) else torch.as_tensor(host)
	t = bufs.get(name)
	if t is None:
		bufs[name] = t = torch.empty(host.shape, dtype=host.dtype, device=device)
	assert tuple(t.shape) == tuple(host.shape) and t.dtype == host.dtype, (name, tuple(t.shape), tuple(host.shape), t.dtype, host.dtype)
	t.copy_(host)
	return t


def scratch(bufs, name, nbytes, device="cuda"):
	"""A private 256-byte aligned uint8 workspace of nbytes, allocated once (by the first eager call, outside any capture)."""
	t = bufs.get(name)
	if t is None:
		assert nbytes > 0, (name, nbytes)
		raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
		off = (-raw.data_ptr()) % 256
		bufs[name] = t = raw[off:off + nbytes]
	assert t.numel() == nbytes, (name, t.numel(), nbytes)
	return t


def poison(t, byte):
	"""Every byte of t <- byte (a device tensor, a view of one with a row pitch, or pinned host memory)."""
	if t.is_contiguous():
		t.view(torch.uint8).fill_(byte)
		return
	p = torch.empty(t.shape, dtype=t.dtype, device=t.device)
	p.view(torch.uint8).fill_(byte)
	t.copy_(p)


def raw_bits(t):
	"""A host copy of t as bytes: two results are equal iff every bit is (NaN payloads and the sign of zero included)."""
	return t.detach().cpu().contiguous().view(torch.uint8).clone()


def shared_scratch(ops):
	"""The grow-only scratch buffers the wrappers of anncur_amd.ops hand to the library when the caller gives none: workspaces like any other."""
	out = []
	for cls in (ops._Workspace, ops._ScoreScratch, ops._ByteScratch):
		out.extend(cls._bufs.values())
	return out


def _workspaces(case, bufs, ops):
	fn = getattr(case, "workspaces", None)
	ws = list(fn(bufs)) if fn is not None else [t for n, t in bufs.items() if n.startswith("ws")]
	return ws + shared_scratch(ops)


def _canon(case, outs):
	outs = list(outs)
	fn = getattr(case, "canon", None)
	return list(fn(outs)) if fn is not None else outs


def run(case, ops):
	"""Steps 1-6 of the procedure; raises AssertionError with the case's name, the data set and the output that differs."""
	bufs = {}
	data = [case.make(0), case.make(1)]
	want = []
	# 1, 2: eager on A and on B -- code objects, dynamic-LDS attributes and the grow-only scratch are warm before the capture; each result
	#       against the host reference, so that "replay == eager" cannot mean "both wrong"
	for d in data:
		case.load(d, bufs)
		outs = case.call(bufs)
		torch.cuda.synchronize()
		host = [o.detach().cpu().clone() for o in _canon(case, outs)]
		case.check(d, host)
		want.append([raw_bits(o) for o in host])
	# 3: a stale output cannot pass
	differ = getattr(case, "differ", None)
	for j, (a, b) in enumerate(zip(want[0], want[1])):
		if differ is None or j in differ:
			assert not torch.equal(a, b), f"{case.name}: output {j} is the same for data sets A and B: a stale result would pass"
	# 4: capture on A
	case.load(data[0], bufs)
	torch.cuda.synchronize()
	g = torch.cuda.CUDAGraph()
	with torch.cuda.graph(g, capture_error_mode="thread_local"):
		outs = list(case.call(bufs))
	# 5, 6: replay on B, then on A again
	for which in (1, 0):
		case.load(data[which], bufs)
		for o in outs:
			poison(o, OUT_POISON)
		for w in _workspaces(case, bufs, ops):
			poison(w, WS_POISON)
		torch.cuda.synchronize()
		g.replay()
		torch.cuda.synchronize()
		typed = [o.detach().cpu().contiguous() for o in _canon(case, outs)]
		got = [raw_bits(o) for o in typed]
		assert len(got) == len(want[which])
		for j, (x, y) in enumerate(zip(got, want[which])):
			if not torch.equal(x, y):
				bad = int((x != y).sum())
				size = typed[j].element_size()
				where = sorted(set((torch.nonzero(x != y)[:8, 0] // size).tolist()))
				flat, eager = typed[j].reshape(-1), y.view(typed[j].dtype).reshape(-1)
				raise AssertionError(f"{case.name}: replay on data set {'AB'[which]}: output {j} differs from the eager result in {bad} of {x.numel()} bytes"
									 f" ({int((x == OUT_POISON).sum())} bytes still hold the output poison); first elements {where}: replay "
									 f"{[flat[i].item() for i in where]}, eager {[eager[i].item() for i in where]}")
	del g
