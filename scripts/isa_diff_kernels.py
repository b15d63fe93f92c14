"""Dev tool: compare the kernels of two builds of the library (or of one object file each), kernel by kernel -- the instruction listings
after replacing register numbers (v12, s[4:5] -> v#, s#) and the resource notes (VGPRs, AGPRs, SGPRs, spills, scratch).  Says for every
kernel whether the listings are identical, differ only BEFORE the first v_mfma (the prologue), or differ behind it; behind it a scalar
load whose offset alone differs and a branch (or the s_add of a far branch) whose displacement alone differs are counted apart.
Compares listings and reads notes, nothing else.
usage: python scripts/isa_diff_kernels.py old.so new.so [name-regex] [--md]"""
import difflib, os, re, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_tools import disassemble, functions, kernel_notes
from check_kernel_resources import parse_kernel_notes

RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")
# template parameters that went away: old spelling -> new spelling of the same kernel
RENAMES = [(r"score_kernel<(\d+), 0, (\d+), false, false, (\d+)>", r"score_prepass_kernel<\1, \2, \3>"),
		   (r"score_kernel<(\d+), 1, 16, (\w+), false, (\d+)>", r"score_sweep_kernel<\1, \2, \3>"),
		   (r"score16_kernel<(\d+), 4>", r"score16_kernel<\1>")]


def demangle(names):
	out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
	res = {}
	for n, d in zip(names, out):
		d = re.sub(r"^void |\(.*\)( \[clone.*)?$", "", d.replace("(anonymous namespace)::", ""))   # (return type and argument list off)
		for a, b in RENAMES: d = re.sub(a, b, d)
		res[n] = d
	return res


def regs(ins):
	return re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", ins)


def loose(ins):
	"""Second normalisation, for the allowed exceptions: the offset of a scalar load, the displacement of a branch (far branch: the literal of its s_add)."""
	if re.match(r"s_load_|s_c?branch|s_add_u32|s_addc_u32", ins): return re.sub(r"(0x[0-9a-f]+|\b\d+)( <.*>)?$", "#", ins)
	return ins


def load(lib):
	kern = {}
	for dis in disassemble(lib):
		for name, body in functions(dis):
			# (zero words behind the last instruction pad the gap to the next function: the disassembler prints them as v_cndmask_b32 v0, s0, v0, vcc)
			while body and re.search(r":\s*00000000\s*$", body[-1][2]): body = body[:-1]
			kern[name] = [regs(ins) for _, ins, _ in body]
	notes = {k[".name"]: k for text in kernel_notes(lib) for k in parse_kernel_notes(text)}
	dm = demangle(sorted(notes))
	return {dm[n]: (kern[n], notes[n]) for n in notes if n in kern}


def verdict(a, b):
	if a == b: return "identical"
	fa = next((i for i, x in enumerate(a) if x.startswith("v_mfma")), len(a))
	fb = next((i for i, x in enumerate(b) if x.startswith("v_mfma")), len(b))
	late = moved = 0
	for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
		if tag == "equal" or (i2 <= fa and j2 <= fb): continue
		if tag == "replace" and i2 - i1 == j2 - j1 and all(loose(x) == loose(y) for x, y in zip(a[i1:i2], b[j1:j2])): moved += i2 - i1
		else: late += 1
	if late: return f"DIFFERS behind the first MFMA ({late} hunks)"
	return "prologue only" + (f" (+ {moved} load offsets / branch displacements)" if moved else "")


if __name__ == "__main__":
	args = [x for x in sys.argv[1:] if x != "--md"]
	old, new, pat = load(args[0]), load(args[1]), re.compile(args[2] if len(args) > 2 else ".")
	row = "| `%s` | %d | %d | %s | %s |" if "--md" in sys.argv else "%-60s %5d -> %5d  %-50s %s"
	for name in sorted(set(old) | set(new)):
		if not pat.search(name): continue
		if name not in old or name not in new:
			print(name, "only in the", "old" if name in old else "new", "build")
			continue
		(a, na), (b, nb) = old[name], new[name]
		dr = ["%s %d -> %d" % (f[1:], na.get(f, 0), nb.get(f, 0)) for f in RES if na.get(f, 0) != nb.get(f, 0)]
		print(row % (name, len(a), len(b), verdict(a, b), "; ".join(dr) if dr else "resources equal (vgpr %d)" % nb.get(".vgpr_count", 0)))
