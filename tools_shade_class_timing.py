#!/usr/bin/env python3
"""Condense an A/B of the headline frame -- the parent commit's library against this tree's, run alternately in one GPU visit --
into profiles/shade_class_timing.json: every run's frame_ms, the exclusive tracer ms of the --full runs, the spreads, the
verdict by the rule of the material-class change (the worst run of the change beats the best of the parent AND the difference of
the means is at least three times the larger spread), and k_wavefront's counters per frame before and after.
usage: python tools_shade_class_timing.py <dir with parent_<i>.json / change_<i>.json / parent_full*.json / change_full*.json bench lines>
                                          <prof dir of the parent> <prof dir of the change>      (tools_profile_run.sh outputs)"""
import collections
import csv
import glob
import json
import os
import sys

ab, prof_parent, prof_change = sys.argv[1:4]


def lines(pat):
    return [json.load(open(f)) for f in sorted(glob.glob(os.path.join(ab, pat)))]


def side(name):
    plain = [d["ms_per_step"] for d in lines(f"{name}_[0-9]*.json")]
    full = lines(f"{name}_full*.json")
    tracer = [d["roofline"]["kernels"]["k_wavefront+k_bounce"]["ms_per_frame"] for d in full]
    gather = [d["roofline"]["kernels"]["k_gather"]["ms_per_frame"] for d in full]
    return {"frame_ms": plain, "frame_ms_mean": round(sum(plain) / len(plain), 4), "frame_ms_spread": round(max(plain) - min(plain), 4),
            "full_run_frame_ms": [d["ms_per_step"] for d in full], "tracer_exclusive_ms": tracer, "gather_exclusive_ms": gather,
            "rays_per_frame": full[0].get("rays_per_frame") if full else None}


def wavefront_counters(prof):
    """k_wavefront's counters summed over the launches of the ONE profiled frame, each from the pass that collected it"""
    out = {}
    for f in glob.glob(os.path.join(prof, "pmc_sq*", "*counter_collection.csv")):
        agg, disp = collections.defaultdict(float), set()
        for r in csv.DictReader(open(f)):
            if r["Kernel_Name"].replace("void ", "").startswith("k_wavefront"):
                agg[r["Counter_Name"]] += float(r["Counter_Value"])
                disp.add(r["Dispatch_Id"])
        for k, v in agg.items():
            out[k] = int(v)
        out["launches"] = len(disp)
    for f in glob.glob(os.path.join(prof, "stats", "*kernel_stats.csv")):
        for r in csv.DictReader(open(f)):
            if r["Name"].replace("void ", "").startswith("k_wavefront"):
                out["stats_pass"] = {"calls": int(r["Calls"]), "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3)}
    keep = ("launches", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU", "stats_pass")
    return {k: out[k] for k in keep if k in out}


P, Cg = side("parent"), side("change")
spread = max(P["frame_ms_spread"], Cg["frame_ms_spread"])
diff = round(P["frame_ms_mean"] - Cg["frame_ms_mean"], 4)
cp, cc = wavefront_counters(prof_parent), wavefront_counters(prof_change)
res = {
    "what": "tools_shade_class_timing.py",
    "command": "python bench.py --gpus 1 --steps 20 --warmup 5 (frame_ms); the same with --full --no-cpu-baseline (exclusive kernel ms, one chunk in flight); "
               "parent and change alternately in one GPU visit, each run a process of its own",
    "parent": P, "change": Cg,
    "mean_difference_ms": diff, "larger_spread_ms": spread,
    "worst_change_beats_best_parent": max(Cg["frame_ms"]) < min(P["frame_ms"]),
    "difference_at_least_3_spreads": diff >= 3 * spread,
    "k_wavefront_counters_per_frame": {"command": "tools_profile_run.sh <tag> stats,sq: rocprofv3 --kernel-trace [--stats | --pmc <4 counters>], one pass each, one profiled frame",
                                       "parent": cp, "change": cc},
}
res["gain"] = bool(res["worst_change_beats_best_parent"] and res["difference_at_least_3_spreads"])
if "SQ_INSTS_VALU" in cp and "SQ_INSTS_VALU" in cc:
    res["k_wavefront_counters_per_frame"]["SQ_INSTS_VALU_ratio"] = round(cc["SQ_INSTS_VALU"] / cp["SQ_INSTS_VALU"], 4)
os.makedirs("profiles", exist_ok=True)
json.dump(res, open("profiles/shade_class_timing.json", "w"), indent=1)
print(json.dumps(res, indent=1))
