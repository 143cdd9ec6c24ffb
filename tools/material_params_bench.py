#!/usr/bin/env python3
"""TRC_FLAG_MATERIAL_PARAMS measured (profiles/r32/material_params.txt), 1920 x 1080 on one MI355X.

The price of the table: a flagged launch of --spp samples with a table of trc_host_default_material_params (the unflagged picture, bit
for bit) against the UNFLAGGED launch forced onto the same shape (knobs no_dense / no_pwg, strip length 1, primary replay off: what the
table fetch and the general divisions cost) and against the production unflagged launch (what a host pays today), on config 2 under
tracePath and traceMIS and on config 4 under tracePath.  One context per side, each with its own settled block costs; the sides take turns
launch by launch, the order reversed every other round; --warmup launches, then medians, minima and maxima of --reps.  Render-kernel time
from the launches' event pairs (trc_stats.kernel_ms) and wall time between two trc_synchronize.  Every side's frame is compared with the
production one's: the same bits."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workloads  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402

W, H = workloads.W, workloads.H
NAMES = {abi.INTEGRATOR_MIS: "traceMIS", abi.INTEGRATOR_PATH: "tracePath"}
OUT = []


def say(text=""):
    print(text, flush=True)
    OUT.append(text)


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return f"{med(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def launch(t, a, integrator, flagged):
    t.seed(a.seed); t.clear_accum(); t.reset_stats()
    t.synchronize()
    t0 = time.perf_counter()
    t.render(spp=a.spp, integrator=integrator, material_params=flagged)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3, t.stats().kernel_ms


def table_cost(a, config, integrator):
    wl = workloads.make(config)
    view = wl["scene"].view
    sides = [("flagged, default table", True, True), ("unflagged, same shape", False, True), ("unflagged, production", False, False)]
    ctxs, res, frames = [], {}, {}
    try:
        for name, flagged, forced in sides:
            t = Tracer(0)
            ctxs.append(t)
            workloads.setup(t, wl)
            if forced:
                for knob in ("no_dense", "no_pwg", "no_primary_replay"):
                    t.debug_set(knob, 1)
                t.debug_set("strip_len", 1)
            if flagged:
                t.upload_material_params(host.default_material_params([view.materials[i].type for i in range(view.n_material)]))
        say(f"--- {wl['what'].split(',')[0]}, {NAMES[integrator]}, {W}x{H}, {a.spp} spp per launch; {a.warmup} warm-up launches, medians of {a.reps}")
        for r in range(a.warmup + a.reps):
            order = list(zip(sides, ctxs))
            for (name, flagged, _), t in (order if r % 2 == 0 else order[::-1]):
                wall, kernel = launch(t, a, integrator, flagged)
                if r >= a.warmup:
                    e = res.setdefault(name, dict(wall=[], kernel=[]))
                    e["wall"].append(wall); e["kernel"].append(kernel)
        for (name, _, _), t in zip(sides, ctxs):
            frames[name] = t.download_accum().view(np.uint32)
        base, prod = med(res[sides[1][0]]["kernel"]), med(res[sides[2][0]]["kernel"])
        for name, _, _ in sides:
            e = res[name]
            same = np.array_equal(frames[name], frames[sides[2][0]])
            say(f"   {name:24s} render kernel {spread(e['kernel'])}  wall {spread(e['wall'])}  x{med(e['kernel']) / base:5.3f} of the same shape, "
                f"x{med(e['kernel']) / prod:5.3f} of production; frame {'==' if same else '!='} production's")
    finally:
        for t in ctxs:
            t.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="2:path,2:mis,4:path", help="config:integrator, comma separated")
    ap.add_argument("--out", default=None, help="write the report here as well")
    a = ap.parse_args()
    integ = {"path": abi.INTEGRATOR_PATH, "mis": abi.INTEGRATOR_MIS}
    for case in a.cases.split(","):
        config, name = case.split(":")
        table_cost(a, config, integ[name])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
