#!/usr/bin/env python3
"""What asking for a NUMBER of g points costs on the FSCK find_g_points job of BASELINE configs[1] (ecckd_amd/fsck_job.py: six
gases, 7.2e6 points, one band): the gases are prepared once, then api.find_g_gases_target looks for the tolerance scaling that
gives 16, 32 and 64 g points, the first guess being the job's own tolerance.  Per trial: seconds, wavenumber points the
searches asked for and points actually swept on the device (the gases' memos of interval errors carry over from trial to
trial).  Per target: the total against ntrial x one plain search of the same prepared gases (memo reset, timed here) and against
ntrial x the whole plain job (--job-seconds: preparation included).

    python tools/target_probe.py [--nwav 7200000] [--targets 16,32,64] [--out profiles/target_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nwav", type=int, default=7_200_000)
    ap.add_argument("--nlay", type=int, default=54)
    ap.add_argument("--tolerance", type=float, default=0.0161)
    ap.add_argument("--tolerance-tolerance", type=float, default=0.01)
    ap.add_argument("--max-iterations", type=int, default=60)
    ap.add_argument("--nlines", type=int, default=12000)
    ap.add_argument("--ngas", type=int, default=6)
    ap.add_argument("--targets", default="16,32,64")
    ap.add_argument("--resolution", type=float, default=1e-3)
    ap.add_argument("--max-trials", type=int, default=40)
    ap.add_argument("--plain-repeats", type=int, default=3)
    ap.add_argument("--job-seconds", type=float, default=3.05, help="one plain job, preparation included (DESIGN 7.0: 3.0-3.1 s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ecckd_amd import api, fsck_job
    ctx = api.Context(0)
    job = fsck_job.FsckJob(ctx, args.nwav, args.nlay, ngas=args.ngas, nlines=args.nlines)
    t0 = time.perf_counter()
    gases = job.prepare()
    ctx.synchronize()
    out = {"nwav": args.nwav, "nlay": args.nlay, "gases": job.names, "first_guess": args.tolerance, "resolution": args.resolution,
           "preparation_s": time.perf_counter() - t0, "job_seconds": args.job_seconds, "plain_search_s": [], "targets": []}

    def stats():
        s = [g.eval_stats() for g in gases]
        return sum(x["points_requested"] for x in s), sum(x["points_evaluated"] for x in s)

    # one plain search of the prepared gases, memo reset every time: the unit a trial is measured in
    for _ in range(args.plain_repeats):
        for g in gases:
            g.reset_memo()
        ctx.synchronize()
        t0 = time.perf_counter()
        res = job.search(gases, args.tolerance, args.tolerance_tolerance, args.max_iterations)
        out["plain_search_s"].append(time.perf_counter() - t0)
    out["plain_ng"] = 1 - len(gases) + sum(len(r[0]["error"]) for r in res)
    out["plain_points_swept"] = stats()[1]
    plain = min(out["plain_search_s"])
    print(json.dumps({k: out[k] for k in ("preparation_s", "plain_search_s", "plain_ng", "plain_points_swept")}), flush=True)

    req = [dict(ibegin=[0], iend=[args.nwav - 1], heating_rate_tolerance=[args.tolerance], options=[dict(min_g_points=1, max_g_points=256)])
           for _ in gases]
    for target in [int(t) for t in args.targets.split(",")]:
        for g in gases:
            g.reset_memo()
        ctx.synchronize()
        trials = []
        last = [time.perf_counter(), 0.0, 0.0]

        def on_trial(i, scaling, ng, per_gas):
            now, (asked, swept) = time.perf_counter(), stats()
            trials.append({"scaling": scaling, "ng": ng, "ng_per_gas": per_gas, "seconds": now - last[0],
                           "points_requested": asked - last[1], "points_swept": swept - last[2]})
            last[:] = [now, asked, swept]

        t0 = time.perf_counter()
        res, info = api.find_g_gases_target(gases, req, 1 - len(gases), target, args.resolution, args.max_trials, args.tolerance_tolerance,
                                            args.max_iterations, on_trial=on_trial)
        total = time.perf_counter() - t0
        asked, swept = stats()
        n = len(trials)
        rec = {"target": target, "status": info["status"], "ng": info["ng"], "scaling": info["scaling"],
               "tolerance_used": float(info["tolerance_used"][0][0]), "ntrial": n, "total_s": total,
               "rerun_s": total - sum(t["seconds"] for t in trials), "rerun_points_swept": swept - last[2],
               "ntrial_x_plain_search_s": n * plain, "ntrial_x_job_s": n * args.job_seconds,
               "points_requested": asked, "points_swept": swept, "trials": trials}
        out["targets"].append(rec)
        print(json.dumps(rec), flush=True)
    for g in gases:
        g.close()
    job.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
