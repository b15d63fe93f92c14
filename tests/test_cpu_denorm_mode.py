"""The build keeps subnormals: every kernel descriptor of the built library has float_denorm_mode_32 = 3 and float_denorm_mode_16_64 = 3
(the compute_pgm_rsrc1 fields the disassembler prints as .amdhsa_float_denorm_mode_*: sources and results are not flushed), and the FLAGS
line of csrc/Makefile carries no fast-math or flush-denormals option.  tests/test_gpu_subnormal_exact.py holds the kernels to IEEE results
on subnormal data; this gate says why a clean checkout can: nothing else is looked at here."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "anncur_amd", "lib", "libanncur_hip.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

_LISTING = """
lib.so.0.hipv4-amdgcn-amd-amdhsa--gfx950:	file format elf64-amdgpu

Disassembly of section .rodata:

.amdhsa_kernel keeps
	.amdhsa_group_segment_fixed_size 0
	.amdhsa_next_free_vgpr 14
	.amdhsa_float_round_mode_32 0
	.amdhsa_float_denorm_mode_32 3
	.amdhsa_float_denorm_mode_16_64 3
	.amdhsa_exception_fp_denorm_src 0
.end_amdhsa_kernel
.amdhsa_kernel flushes32
	.amdhsa_float_denorm_mode_32 0
	.amdhsa_float_denorm_mode_16_64 3
.end_amdhsa_kernel
.amdhsa_kernel silent
	.amdhsa_next_free_vgpr 8
.end_amdhsa_kernel
	.amdhsa_float_denorm_mode_32 3
"""


def test_parser_reads_the_two_fields_of_every_kernel():
	from isa_tools import denorm_modes
	assert denorm_modes(_LISTING) == {"keeps": (3, 3), "flushes32": (0, 3), "silent": (None, None)}   # (a directive outside a kernel belongs to none)
	assert denorm_modes("") == {}


@pytest.fixture(scope="module")
def built():
	from isa_tools import denorm_modes, kernel_descriptors
	assert os.path.exists(LIB), "build the library first (python __graft_entry__.py)"
	out = {}
	for text in kernel_descriptors(LIB):
		out.update(denorm_modes(text))
	return out


def test_every_kernel_of_the_built_library_keeps_subnormals(built):
	from check_kernel_resources import parse_kernel_notes
	from isa_tools import kernel_notes
	names = {k[".name"] for text in kernel_notes(LIB) for k in parse_kernel_notes(text)}
	assert len(built) >= 100 and set(built) == names, (len(built), len(names))            # every kernel the metadata lists has a descriptor here
	bad = {k: v for k, v in built.items() if v != (3, 3)}
	assert not bad, f"{len(bad)} kernels flush subnormals (float_denorm_mode_32, float_denorm_mode_16_64): {dict(list(bad.items())[:5])}"


def test_makefile_flags_carry_no_flushing_option():
	with open(os.path.join(ROOT, "anncur_amd", "csrc", "Makefile")) as f:
		lines = [l for l in f.read().splitlines() if re.match(r"^FLAGS\s*[:?+]?=", l)]
	assert len(lines) == 1, lines
	for opt in lines[0].split():
		assert not re.search(r"fast-math|-Ofast|fgpu-flush-denormals-to-zero|denormal-fp-math|-fcuda-flush|unsafe-math|-cl-denorms-are-zero|-ffp-model=fast", opt), opt
