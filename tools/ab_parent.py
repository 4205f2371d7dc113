"""This tree's library against another build of it -- usually the parent commit's, made beside it with `make variant NAME=parent`
-- on one GPU, in alternating fresh processes: the benchmark's step time and tools/frame_times.py's single frames.  Every run and
the summary go to one JSON file (DESIGN.md section 8 names the checks the summary answers).  A child that ends abnormally ends the run.
usage: python tools/ab_parent.py --parent simd-raytracer_amd/build_parent/librtk_hip.so --out profiles/NAME.json
       [--bench 7] [--steps 200] [--warmup 20] [--frame-procs 3] [--frames 192] [--parent-cap 0] [--parent-judged 0]
The frames that carry a sort or a judge are worked out from the schedule each side runs under: RTK_COST_RESORT_EVERY / _MAX /
RTK_COST_JUDGE of the environment for this tree's library, --parent-cap / --parent-judged for the other one."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(cmd, lib, limit):
    env = dict(os.environ)
    env.pop("RTK_LIB_OVERRIDE", None)
    if lib:
        env["RTK_LIB_OVERRIDE"] = os.path.abspath(lib)
    res = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"{' '.join(cmd)} (lib {lib or 'this tree'}) ended with {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def sort_frames(n, every=16, cap=0):
    """1-based frames that start a new list under frame_plan.hpp's schedule (cap 0: every `every` frames)."""
    out, f, sorts = [], 2, 0
    while f <= n:
        out.append(f)
        sorts += 1
        iv = every
        for _ in range(3, sorts + 1):
            if iv < cap:
                iv *= 2
        f += min(iv, cap) if cap > every else every
    return out


def schedule_of(side, a):
    """(resort_every, cap, judged) of a side's library: what the children run under.  The knobs of the environment reach both
    sides; a library from before the cap ignores it (--parent-cap 0, --parent-judged 0: the defaults)."""
    every_env, cap_env = os.environ.get("RTK_COST_RESORT_EVERY"), os.environ.get("RTK_COST_RESORT_MAX")
    every = int(every_env) if every_env else 16
    if side == "parent":
        return every, a.parent_cap, bool(a.parent_judged)
    cap = int(cap_env) if cap_env else (0 if every_env else 128)       # (accel.hpp: an interval that is asked for is not stretched)
    return every, cap, os.environ.get("RTK_COST_JUDGE", "1") != "0"


def frame_summary(runs, first, threshold_of, schedules):
    """Per side: the frames from `first` on that carry neither a sort nor a judge, by segment (the frames of one list)."""
    per_side = {}
    for side, procs in runs.items():
        every, cap, judged = schedules[side]
        rows = []
        for p in procs:
            n = len(p["ms"])
            starts = sort_frames(n + 1, every, cap)
            carrying = {s - 1 for s in starts} | ({s for s in starts if s > 2} if judged else set()) | {2}
            segs = []
            for k, s in enumerate(starts):
                end = starts[k + 1] - 1 if k + 1 < len(starts) else n
                fr = [f for f in range(max(s, first), end + 1) if f not in carrying]
                if fr:
                    segs.append({"first": fr[0], "last": fr[-1], "median_ms": statistics.median(p["ms"][f - 1] for f in fr), "frames": fr})
            rows.append(segs)
        per_side[side] = rows
    fastest = min(seg["median_ms"] for rows in per_side.values() for segs in rows for seg in segs)
    limit = threshold_of * fastest
    out = {"first_frame": first, "fastest_segment_median_ms": fastest, "slow_above_ms": limit,
           "schedules": {side: {"resort_every": v[0], "resort_max": v[1], "judged": v[2]} for side, v in schedules.items()}}
    for side, rows in per_side.items():
        procs = []
        for p, segs in zip(runs[side], rows):
            fr = [f for seg in segs for f in seg["frames"]]
            slow = [f for f in fr if p["ms"][f - 1] > limit]
            procs.append({"frames": len(fr), "slow": len(slow), "share": len(slow) / len(fr),
                          "segment_medians_ms": [[seg["first"], seg["last"], round(seg["median_ms"], 4)] for seg in segs],
                          "sort_and_judge_frames_ms": {str(f): p["ms"][f - 1] for f in range(first, len(p["ms"]) + 1) if f not in set(fr)},
                          "judge": p.get("judge")})
        total, slow = sum(q["frames"] for q in procs), sum(q["slow"] for q in procs)
        out[side] = {"share_slow": slow / total, "frames": total, "slow": slow, "processes": procs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--bench", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frame-procs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--parent-cap", type=int, default=0, help="RTK_COST_RESORT_MAX as the parent library understands it (0: it has none)")
    ap.add_argument("--parent-judged", type=int, default=0, help="1: the parent library judges its new lists too")
    a = ap.parse_args()
    libs = {"parent": a.parent, "new": None}
    result = {"what": "the parent commit's library against this tree's on one GPU, alternating fresh processes",
              "command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}"}
    runs = {"parent": [], "new": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def save():                                            # (after every child: a run that is cut short leaves what it had)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    for i in range(a.bench):
        for side in ("parent", "new"):
            r = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)], libs[side], 240)
            runs[side].append(r)
            result["bench_lines"] = runs
            save()
            print(f"bench {i} {side}: {r.get('ms_per_step')}", flush=True)
    if a.bench:
        ms = {s: [r["ms_per_step"] for r in runs[s]] for s in runs}
        result["ms_per_step"] = {s: {"runs": ms[s], "median": statistics.median(ms[s]), "min": min(ms[s]), "max": max(ms[s])} for s in ms}
        p, n = result["ms_per_step"]["parent"], result["ms_per_step"]["new"]
        result["ms_per_step"]["checks"] = {"new_median_below_parent_fastest": n["median"] < p["min"],
                                           "median_difference": p["median"] - n["median"], "parent_spread": p["max"] - p["min"],
                                           "difference_above_parent_spread": p["median"] - n["median"] > p["max"] - p["min"]}
    ft = {"parent": [], "new": []}
    for i in range(a.frame_procs):
        for side in ("parent", "new"):
            r = child([sys.executable, "tools/frame_times.py", "0", str(a.frames)], libs[side], 240)
            ft[side].append(r)
            result["frame_times"] = {"runs": ft}
            save()
            print(f"frame_times {i} {side}: median {r['median_ms']:.4f}", flush=True)
    if a.frame_procs:
        result["frame_times"] = {"summary": frame_summary(ft, 35, 1.08, {side: schedule_of(side, a) for side in ft}), "runs": ft}
        s = result["frame_times"]["summary"]
        s["new_share_at_most_half_of_parent"] = s["new"]["share_slow"] <= 0.5 * s["parent"]["share_slow"]
    save()
    print(json.dumps({k: v for k, v in result.items() if k in ("ms_per_step",)} | {"frame_times": {k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "processes"})
                      for k, v in result.get("frame_times", {}).get("summary", {}).items()}}, indent=1)[:6000])


if __name__ == "__main__":
    main()
