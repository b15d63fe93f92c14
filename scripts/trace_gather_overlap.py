"""Dev tool: does the next step's column gather run beside the sweep?  From a rocprofv3 --kernel-trace CSV of `bench.py --direct`
(nothing else enabled), over the last N steps (the timed ones; a step = one gather_cols_kernel dispatch):
  * the share of gather_cols_kernel dispatches that BEGIN before the previous score16_kernel dispatch ENDS, and how much of the gather
    lies inside that sweep;
  * the median gap from a sweep's end to the next prepass16_kernel's start;
  * median durations of the gather, the sweep and the prepass.
One JSON line.  usage: python scripts/trace_gather_overlap.py <kernel_trace.csv> [N = 50]"""
import bisect, csv, json, statistics, sys

rows = list(csv.DictReader(open(sys.argv[1])))
n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50


def of(name):
	out = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?")) for r in rows if name in r["Kernel_Name"])
	return out


gathers, sweeps, prepasses = of("gather_cols_kernel"), of("score16_kernel"), of("prepass16_kernel")
gathers = gathers[-n_steps:]
t_first = gathers[0][0]
sweep_starts, prepass_starts = [s[0] for s in sweeps], [p[0] for p in prepasses]
begun, inside_us, queues = 0, [], set()
for gs, ge, gq in gathers:
	j = bisect.bisect_right(sweep_starts, gs) - 1     # the sweep dispatched last before this gather began
	if j < 0: continue
	ss, se, sq = sweeps[j]
	if gs < se:
		begun += 1
		inside_us.append((min(ge, se) - gs) / 1e3)
		queues.add((gq, sq))
gaps = []
for ss, se, _ in sweeps:
	if ss < t_first: continue
	j = bisect.bisect_right(prepass_starts, ss)       # the next prepass after this sweep began
	if j < len(prepasses): gaps.append((prepasses[j][0] - se) / 1e3)
med = lambda xs: round(statistics.median(xs), 2) if xs else None
dur = lambda xs, t0: med([(e - s) / 1e3 for s, e, _ in xs if s >= t0])
print(json.dumps({
	"steps": len(gathers),
	"gathers_begun_before_previous_sweep_ended": begun,
	"share": round(begun / len(gathers), 3),
	"median_us_of_gather_inside_sweep": med(inside_us),
	"queue_pairs_gather_sweep": sorted(queues),
	"median_gap_sweep_end_to_next_prepass_start_us": med(gaps),
	"min_gap_us": round(min(gaps), 2) if gaps else None,
	"median_us": {"gather": dur(gathers, t_first), "sweep": dur(sweeps, t_first), "prepass": dur(prepasses, t_first)},
}))
