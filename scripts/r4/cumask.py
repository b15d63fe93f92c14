"""CU-masked streams for the scan probes of this directory."""
import ctypes

import torch

hip = ctypes.CDLL("libamdhip64.so")


def masked_stream(lo, hi, n_cu=256):
	"""A stream on the CUs whose mask bits are lo .. hi - 1 (ops.cu_partition_streams' call, uncached)."""
	fn = hip.hipExtStreamCreateWithCUMask
	fn.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
	words = (n_cu + 31) // 32
	mask = (ctypes.c_uint32 * words)(*[sum(1 << b for b in range(32) if lo <= 32 * w + b < hi) for w in range(words)])
	h = ctypes.c_void_p()
	rc = fn(ctypes.byref(h), words, mask)
	assert rc == 0 and h.value, rc
	return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", 0))
