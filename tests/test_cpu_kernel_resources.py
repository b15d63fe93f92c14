"""The register / LDS budget of `make verify` (scripts/check_kernel_resources.py, DESIGN.md 4.1 'Register account'): its metadata parser
against the notes of the built library and against hand-written notes, and its verdicts on kernels that have outgrown the budget."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "anncur_amd", "lib", "libanncur_hip.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

_NOTES = """
Displaying notes found in: .note
  Owner                Data size 	Description
  AMDGPU               0x00000a5c	NT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .actual_access:  read_only
        .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         8
        .size:           4
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .kernarg_segment_size: 64
    .max_flat_workgroup_size: 256
    .name:           _ZN12_GLOBAL__N_119overlap_wave_kernelEPKiiS1_ilNS_8OvlPairsEiPi
    .private_segment_fixed_size: 0
    .sgpr_count:     22
    .symbol:         _ZN12_GLOBAL__N_119overlap_wave_kernelEPKiiS1_ilNS_8OvlPairsEiPi.kd
    .uses_dynamic_stack: false
    .vgpr_count:     14
    .vgpr_spill_count: 0
    .wavefront_size: 64
  - .args:
      - .offset:         0
        .size:           8
        .value_kind:     by_value
    .agpr_count:     0
    .group_segment_fixed_size: 1024
    .name:           'other_kernel'
    .private_segment_fixed_size: 0x10
    .uses_dynamic_stack: true
    .vgpr_count:     33
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""


def test_parser_reads_the_top_level_fields_of_every_kernel():
	from check_kernel_resources import allocated_vgprs, parse_kernel_notes
	ks = parse_kernel_notes(_NOTES)
	assert [k[".name"] for k in ks] == ["_ZN12_GLOBAL__N_119overlap_wave_kernelEPKiiS1_ilNS_8OvlPairsEiPi", "other_kernel"]
	a, b = ks
	assert a[".vgpr_count"] == 14 and a[".private_segment_fixed_size"] == 0 and a[".group_segment_fixed_size"] == 0
	assert a[".kernarg_segment_size"] == 64 and a[".uses_dynamic_stack"] is False and a[".sgpr_count"] == 22
	assert ".offset" not in a and ".size" not in a and ".value_kind" not in a        # the fields of .args entries are not the kernel's
	assert b[".vgpr_count"] == 33 and b[".private_segment_fixed_size"] == 16 and b[".group_segment_fixed_size"] == 1024 and b[".uses_dynamic_stack"] is True
	assert parse_kernel_notes("amdhsa.target: x\n") == [] and parse_kernel_notes("") == []
	assert [allocated_vgprs(n) for n in (1, 8, 14, 18, 24, 25, 240, 241, 252)] == [8, 8, 16, 24, 24, 32, 240, 248, 256]


def _kernel(name, vgpr, scratch=0, lds=0, **more):
	return {".name": name, ".vgpr_count": vgpr, ".private_segment_fixed_size": scratch, ".group_segment_fixed_size": lds, **more}


_SWEEP = "_ZN12_GLOBAL__N_114score16_kernelILi256EEEvNS_11FusedParamsE"
_GATHER = "_ZN12_GLOBAL__N_118gather_cols_kernelIttEEvPKT_lllPKiiPT0_l"
_OVERLAP = "_ZN12_GLOBAL__N_119overlap_wave_kernelEPKiiS1_ilNS_8OvlPairsEiPi"


def test_verdicts():
	from check_kernel_resources import check_kernels
	others = [_kernel("_ZN12_GLOBAL__N_114score16_kernelILi128EEEvNS_11FusedParamsE", 300, scratch=64),      # not held to a budget
			  _kernel("_ZN12_GLOBAL__N_118gather_cols_kernelIffEEvPKT_lllPKiiPT0_l", 64, lds=4096)]
	good = [_kernel(_SWEEP, 240), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)] + others
	f, rows = check_kernels(good)
	assert f == [] and [w for w, _ in rows] == ["score16_kernel<256>", "gather_cols_kernel<uint16_t, uint16_t>", "overlap_wave_kernel"]
	assert check_kernels([_kernel(_SWEEP, 233), _kernel(_GATHER, 24, scratch=8), _kernel(_OVERLAP, 24)])[0] == []    # scratch is the sweep's limit only

	def one(ks, word):
		f, _ = check_kernels(ks + others)
		assert len(f) == 1 and word in f[0], f

	one([_kernel(_SWEEP, 241), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "241 VGPRs (248 allocated)")
	one([_kernel(_SWEEP, 252), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "252 VGPRs (256 allocated)")
	one([_kernel(_SWEEP, 240, scratch=16), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "scratch")
	one([_kernel(_SWEEP, 240, **{".vgpr_spill_count": 3}), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "scratch")
	one([_kernel(_SWEEP, 240, **{".uses_dynamic_stack": True}), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "scratch")
	one([_kernel(_SWEEP, 240), _kernel(_GATHER, 25), _kernel(_OVERLAP, 14)], "gather_cols_kernel<uint16_t, uint16_t>: 25 VGPRs")
	one([_kernel(_SWEEP, 240), _kernel(_GATHER, 18, lds=256), _kernel(_OVERLAP, 14)], "256 bytes of LDS")
	one([_kernel(_SWEEP, 240), _kernel(_GATHER, 18), _kernel(_OVERLAP, 26)], "overlap_wave_kernel: 26 VGPRs")
	one([_kernel(_SWEEP, 240), _kernel(_GATHER, 18), _kernel(_OVERLAP, 14, lds=64)], "overlap_wave_kernel: 64 bytes of LDS")
	# a kernel that was renamed or dropped does not pass silently
	one([_kernel(_SWEEP, 240), _kernel(_GATHER, 18)], "overlap_wave_kernel: 0 kernels match")
	one([_kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "score16_kernel<256>: 0 kernels match")
	bad = _kernel(_SWEEP, 240)
	del bad[".private_segment_fixed_size"]
	one([bad, _kernel(_GATHER, 18), _kernel(_OVERLAP, 14)], "no .private_segment_fixed_size")


@pytest.fixture(scope="module")
def built():
	from check_kernel_resources import parse_kernel_notes
	from isa_tools import kernel_notes
	assert os.path.exists(LIB), "build the library first (python __graft_entry__.py)"
	return [k for text in kernel_notes(LIB) for k in parse_kernel_notes(text)]


def test_parser_on_the_built_library(built):
	"""Every kernel of every code object comes out with a name and the three numbers the budget reads; the counts are plausible for
	gfx950 (one 512-entry file per SIMD lane) and the well-known kernels are among them."""
	assert len(built) >= 100, len(built)
	names = [k[".name"] for k in built]
	assert len(set(names)) == len(names)
	for k in built:
		assert 1 <= k[".vgpr_count"] <= 512 and k[".private_segment_fixed_size"] >= 0 and 0 <= k[".group_segment_fixed_size"] <= 163840, k
		assert k[".wavefront_size"] == 64 and isinstance(k[".uses_dynamic_stack"], bool), k
		assert k[".symbol"] == k[".name"] + ".kd"
	for frag in ("14score16_kernelILi64EE", "14score16_kernelILi128EE", "14score16_kernelILi256EE", "16prepass16_kernelILi256EE",
				 "18gather_cols_kernelIttEE", "18gather_cols_kernelIffEE", "19overlap_wave_kernelE"):
		assert sum(frag in n for n in names) == 1, frag


def test_built_library_keeps_the_room_beside_the_sweep(built):
	"""What `make verify` enforces: score16_kernel<256> at 240 VGPRs or fewer without scratch, the column gather and the overlap counts
	at 24 or fewer without LDS -- two sweep waves and one of theirs fit a SIMD's 512 registers."""
	from check_kernel_resources import allocated_vgprs, check, check_kernels
	f, rows = check_kernels(built)
	assert f == [], "\n".join(f)
	sweep, gather, overlap = (k for _, k in rows)
	assert 2 * allocated_vgprs(sweep[".vgpr_count"]) + max(allocated_vgprs(gather[".vgpr_count"]), allocated_vgprs(overlap[".vgpr_count"])) <= 512
	f2, rows2, n = check(LIB)
	assert f2 == [] and n == len(built) and len(rows2) == 3
