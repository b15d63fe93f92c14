"""Shared helpers of the static ISA checks (check_mfma_hazards.py, check_lds_hazards.py, check_kernel_resources.py): extract the gfx950 code objects of a built
library with llvm-objdump --offloading, disassemble them, split the listing into functions of (address, instruction, raw tail)."""
import os, re, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
SMEM = re.compile(r"^\s*(s_load_|s_buffer_load_|s_memtime|s_memrealtime|s_scratch_load|s_atc_probe|s_dcache)")
# (rescore_kernel of split.hip: it was covered as a substring match of the sweep's former name and stays covered)
KERNELS = re.compile(r"ivf_tile128_kernel|score_sweep_kernel|score_prepass_kernel|rescore_kernel|score16_kernel|prepass16_kernel|evalf_kernel|error_lds_kernel|scoreq16_kernel|wide_kernel|error_kernel")


def _code_objects(lib: str, tmp: str):
	"""Unbundle the library's gfx950 code objects into tmp; their file names, sorted."""
	shutil.copy(lib, os.path.join(tmp, "lib.so"))
	subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
	return [f for f in sorted(os.listdir(tmp)) if "amdgcn" in f and os.path.getsize(os.path.join(tmp, f)) > 0]


def disassemble(lib: str):
	tmp = tempfile.mkdtemp(prefix="anncur_co_")
	try:
		return [subprocess.run([f"{LLVM}/llvm-objdump", "-d", f], cwd=tmp, check=True, capture_output=True, text=True).stdout for f in _code_objects(lib, tmp)]
	finally:
		shutil.rmtree(tmp, ignore_errors=True)


def kernel_notes(lib: str):
	"""The metadata notes (llvm-readelf --notes: the amdhsa.kernels list as text) of every code object of the library."""
	tmp = tempfile.mkdtemp(prefix="anncur_co_")
	try:
		return [subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f], cwd=tmp, check=True, capture_output=True, text=True).stdout for f in _code_objects(lib, tmp)]
	finally:
		shutil.rmtree(tmp, ignore_errors=True)


def kernel_descriptors(lib: str):
	"""The kernel descriptors of every code object of the library as llvm-objdump prints them (.amdhsa_kernel NAME ... .end_amdhsa_kernel,
	one .amdhsa_* directive per field of compute_pgm_rsrc1..3)."""
	tmp = tempfile.mkdtemp(prefix="anncur_co_")
	try:
		return [subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-j", ".rodata", f], cwd=tmp, check=True, capture_output=True, text=True).stdout for f in _code_objects(lib, tmp)]
	finally:
		shutil.rmtree(tmp, ignore_errors=True)


def denorm_modes(text: str):
	"""{kernel name: (float_denorm_mode_32, float_denorm_mode_16_64)} of one descriptor listing; None for a field the listing lacks.
	Mode 3 keeps subnormal sources and results, 0 flushes both (compute_pgm_rsrc1 bits 16..19)."""
	out, name = {}, None
	for line in text.splitlines():
		w = line.split()
		if len(w) == 2 and w[0] == ".amdhsa_kernel":
			name = w[1]
			out[name] = [None, None]
		elif w and w[0] == ".end_amdhsa_kernel":
			name = None
		elif name and len(w) == 2 and w[0] in (".amdhsa_float_denorm_mode_32", ".amdhsa_float_denorm_mode_16_64"):
			out[name][w[0].endswith("16_64")] = int(w[1], 0)
	return {k: tuple(v) for k, v in out.items()}


def functions(dis: str):
	name, body = None, []
	for line in dis.splitlines():
		m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
		if m:
			if name: yield name, body
			name, body = m.group(1), []
		elif name and "//" in line:
			ins, _, tail = line.partition("//")
			am = re.match(r"\s*([0-9A-Fa-f]+):", tail)
			if am: body.append((int(am.group(1), 16), ins.strip(), tail))
	if name: yield name, body


def _lgkm(ins: str):
	"""lgkmcnt value of an s_waitcnt (None: the instruction does not wait on lgkmcnt)."""
	if not ins.lstrip().startswith("s_waitcnt"):
		return None
	m = re.search(r"lgkmcnt\((\d+)\)", ins)
	if m:
		return int(m.group(1))
	m = re.search(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s", ins + " ")  # raw immediate: lgkmcnt = bits 8..11
	if m:
		return (int(m.group(1), 0) >> 8) & 0xF
	return None if ("vmcnt" in ins or "expcnt" in ins) else 0


