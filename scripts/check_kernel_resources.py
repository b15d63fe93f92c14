"""Static check of the register / LDS room the sweep leaves on a CU (DESIGN.md 4.1 'Register account'), over the BUILT library.

score16_kernel<256> runs two workgroups per CU, two waves per SIMD.  At 240 VGPRs (allocated in granules of 8) they take 480 of a
SIMD's 512 registers per lane, and the 32 left hold one wave of a small kernel of another stream -- the next step's column gather, the
previous step's overlap counts -- if that kernel allocates at most 24 registers and no LDS (the sweep's two workgroups hold 2 x 79 888
of the CU's 163 840 bytes).  Nothing in the sources says so: `amdgpu_num_vgpr` is ignored by the compiler, the counts are what
register allocation made of the code.  This script reads them from the code objects' metadata notes (`amdhsa.kernels`: .vgpr_count,
.private_segment_fixed_size, .group_segment_fixed_size) and fails when the room is gone.  It reads resource numbers only, never
instructions.

usage: python scripts/check_kernel_resources.py [lib.so]
"""
import os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VGPR_GRANULE, VGPR_FILE = 8, 512
# (regex on the MANGLED kernel name, what it is, most VGPRs, may use scratch, may use static LDS)
LIMITS = [
	(r"14score16_kernelILi256EE", "score16_kernel<256>", 240, False, True),
	(r"18gather_cols_kernelIttEE", "gather_cols_kernel<uint16_t, uint16_t>", 24, True, False),
	(r"19overlap_wave_kernelE", "overlap_wave_kernel", 24, True, False),
]
# A budget of its own: the speculative instantiations of the plain wave-per-row scans.  Four workgroups per CU = four waves per SIMD is what their LDS allows, and
# 128 registers is what four waves leave each.  The restart loop of the speculative start stays there only while the compiler does not hoist
# per-lane addresses out of it: a toolchain that does costs a wave per SIMD without a word, so it fails the build here.
SCAN_LIMITS = [
	(r"24rowwise_topk_wave_kernelIfLb0ELb0ELb0ELi2ELb1EE", "rowwise_topk_wave_kernel<float, pointer loads>", 128, False, True),
	(r"24rowwise_topk_wave_kernelIfLb0ELb1ELb0ELi2ELb1EE", "rowwise_topk_wave_kernel<float, buffer loads>", 128, False, True),
	(r"24rowwise_topk_wave_kernelItLb0ELb0ELb0ELi2ELb1EE", "rowwise_topk_wave_kernel<bf16, pointer loads>", 128, False, True),
	(r"24rowwise_topk_wave_kernelItLb0ELb1ELb0ELi2ELb1EE", "rowwise_topk_wave_kernel<bf16, buffer loads>", 128, False, True),
]
_INT_FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
			   ".group_segment_fixed_size", ".max_flat_workgroup_size", ".wavefront_size", ".kernarg_segment_size")


def parse_kernel_notes(text: str):
	"""The kernels of one code object's notes (llvm-readelf --notes): a list of {field: value} with the top-level fields of each entry of
	`amdhsa.kernels` (.name, .vgpr_count, ...; integers where the field is a count or a size, booleans for true / false).  The list is
	block YAML as LLVM prints it: an entry starts at '  - .field:', its other fields sit at four spaces; nested lists (.args) are skipped."""
	kernels, cur, inside = [], None, False
	for line in text.splitlines():
		if re.match(r"^amdhsa\.kernels:\s*$", line):
			inside = True
			continue
		if not inside:
			continue
		if re.match(r"^\S", line):   # the next top-level key (amdhsa.target, amdhsa.version) or the end of the note
			inside, cur = False, None
			continue
		m = re.match(r"^  - (\.\w+):\s*(.*)$", line)
		if m:
			cur = {}
			kernels.append(cur)
		else:
			m = re.match(r"^    (\.\w+):\s*(.*)$", line)
		if not m or cur is None:
			continue
		key, val = m.group(1), m.group(2).strip().strip("'\"")
		if key in _INT_FIELDS:
			cur[key] = int(val, 0)
		elif val in ("true", "false"):
			cur[key] = val == "true"
		elif val != "":
			cur[key] = val
	return [k for k in kernels if ".name" in k]


def allocated_vgprs(count: int) -> int:
	return -(-count // VGPR_GRANULE) * VGPR_GRANULE


def check_kernels(kernels, limits=None):
	"""Findings (strings) for a list of parsed kernels, and the rows that were judged [(what, kernel)].  limits: LIMITS (the room beside the
	sweep, with the sum over a SIMD) unless given -- SCAN_LIMITS are per-kernel limits only."""
	findings, rows = [], []
	beside_sweep = limits is None
	for pat, what, max_vgpr, scratch_ok, lds_ok in (LIMITS if beside_sweep else limits):
		hit = [k for k in kernels if re.search(pat, k[".name"])]
		if len(hit) != 1:
			findings.append(f"{what}: {len(hit)} kernels match (expected one)")
			continue
		k = hit[0]
		rows.append((what, k))
		missing = [f for f in (".vgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size") if f not in k]
		if missing:
			findings.append(f"{what}: the metadata has no {', '.join(missing)}")
			continue
		if k[".vgpr_count"] > max_vgpr:
			findings.append(f"{what}: {k['.vgpr_count']} VGPRs ({allocated_vgprs(k['.vgpr_count'])} allocated), at most {max_vgpr} leave the room")
		if not scratch_ok and (k[".private_segment_fixed_size"] or k.get(".vgpr_spill_count", 0) or k.get(".uses_dynamic_stack", False)):
			findings.append(f"{what}: scratch ({k['.private_segment_fixed_size']} bytes per lane, {k.get('.vgpr_spill_count', 0)} spills)")
		if not lds_ok and k[".group_segment_fixed_size"]:
			findings.append(f"{what}: {k['.group_segment_fixed_size']} bytes of LDS; beside two sweep workgroups a CU has none to give")
	if not findings and beside_sweep:   # the sum the limits stand for: two sweep waves and one guest per SIMD
		sweep = allocated_vgprs(rows[0][1][".vgpr_count"])
		for what, k in rows[1:]:
			if 2 * sweep + allocated_vgprs(k[".vgpr_count"]) > VGPR_FILE:
				findings.append(f"{what}: 2 x {sweep} + {allocated_vgprs(k['.vgpr_count'])} registers exceed the SIMD's {VGPR_FILE}")
	return findings, rows


def check(lib, limits=None):
	"""(findings, rows judged, kernels in the metadata) of a built library against LIMITS, or against `limits` (SCAN_LIMITS)."""
	from isa_tools import kernel_notes
	kernels = [k for text in kernel_notes(lib) for k in parse_kernel_notes(text)]
	return check_kernels(kernels, limits) + (len(kernels),)


if __name__ == "__main__":
	lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anncur_amd", "lib", "libanncur_hip.so")
	f, rows, n = check(lib)
	f_scan, rows_scan, _ = check(lib, SCAN_LIMITS)
	f, rows = f + f_scan, rows + rows_scan
	print(f"{lib}: {n} kernels in the metadata, {len(rows)} held to a register / LDS budget, {len(f)} findings")
	for what, k in rows:
		print("  %-40s vgpr %3d (allocated %3d) scratch %d lds %d" % (what, k[".vgpr_count"], allocated_vgprs(k[".vgpr_count"]), k[".private_segment_fixed_size"], k[".group_segment_fixed_size"]))
	for x in f: print("  " + x)
	sys.exit(1 if f else 0)
