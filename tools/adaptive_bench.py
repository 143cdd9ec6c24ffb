#!/usr/bin/env python3
"""trc_render_adaptive measured (profiles/r28/adaptive_sampling.txt).

Scenes: config 2 (Cornell box + 12 spheres) and Cornell + the replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, device-built
SAH tree with triangle leaves), 1920 x 1080, traceMIS and tracePath.
  0. the default threshold: the median E_t of config 2 under traceMIS at n = 64 with A at 32 (include/tracer_abi.h takes it from here).
  1. per round, each on its own (wall time between two trc_synchronize, medians of --reps): trc_tile_error with the snapshot -- against the
     48 bytes per pixel of the active tiles it moves --, the read-back of one value per tile, and a mask that clears every second tile with
     the list rebuilt at once, costs carried and (knob mask_forgets_costs) forgotten.  The decision kernel has no entry point of its own:
     it is one thread per tile between the two.
  2. the whole call: trc_render_adaptive at --threshold (default: the library's) and max_spp 256 against uniform renders of 64, 128 and 256
     samples, alternated in one process: wall time, samples spent, RMSE against a --truth-spp frame of another seed rendered here, and
     the histogram of n_t over the tiles.
  3. the same adaptive call with knob mask_forgets_costs, alternated with the carried costs."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402
from update_vertices_bench import FLAGS, med  # noqa: E402

NAMES = {abi.INTEGRATOR_MIS: "traceMIS", abi.INTEGRATOR_PATH: "tracePath"}
OUT = []


def say(text=""):
    print(text, flush=True)
    OUT.append(text)


def timed(t, fn):
    t.synchronize()
    t0 = time.perf_counter()
    fn()
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return f"{med(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def fresh(t, seed):
    t.seed(seed); t.clear_accum(); t.reset_stats()


def default_threshold(t, a):
    fresh(t, a.seed)
    t.render(spp=32, integrator=abi.INTEGRATOR_MIS); t.tile_snapshot(); t.render(spp=32, integrator=abi.INTEGRATOR_MIS, frame0=32)
    t.tile_error()
    e = np.sort(t.tile_errors().ravel())
    q = lambda f: float(e[int(f * (len(e) - 1))])
    say(f"0. config 2, traceMIS, {a.width}x{a.height}, E_t at n = 64 with A at 32 over {len(e)} tiles: min {e[0]:.5f}, quartile {q(0.25):.5f}, "
        f"MEDIAN {float(np.median(e)):.5f}, quartile {q(0.75):.5f}, 95 % {q(0.95):.5f}, max {e[-1]:.5f}")
    return float(np.median(e))


def per_round(t, a, integrator):
    W, H = a.width, a.height
    th, tw = t.tile_grid()
    fresh(t, a.seed)
    t.render(spp=32, integrator=integrator); t.tile_snapshot(); t.render(spp=32, integrator=integrator, frame0=32)
    err = [timed(t, lambda: t.tile_error(snapshot_after=True)) for _ in range(a.reps + 2)][2:]
    back = [timed(t, t.tile_errors) for _ in range(a.reps + 2)][2:]
    half = (np.indices((th, tw)).sum(axis=0) % 2 == 0).astype(np.uint8)
    t.set_tile_mask(half)
    err_half = [timed(t, lambda: t.tile_error(snapshot_after=True)) for _ in range(a.reps + 2)][2:]
    t.set_tile_mask(None)
    gbs = lambda ms, px: 48.0 * px / (ms * 1e-3) / 1e9
    px_half = int(np.repeat(np.repeat(half, 16, 0), 16, 1)[:H, :W].sum())
    say(f"   trc_tile_error + snapshot, every tile      {spread(err)}   48 B x {W * H} px: {gbs(med(err), W * H):7.1f} GB/s")
    say(f"   trc_tile_error + snapshot, every 2nd tile  {spread(err_half)}   48 B x {px_half} px: {gbs(med(err_half), px_half):7.1f} GB/s")
    say(f"   read-back of one float per tile ({th * tw})    {spread(back)}")
    for knob in (0, 1):
        t.debug_set("mask_forgets_costs", knob)
        rebuild = []
        for _ in range(a.reps + 2):
            t.set_tile_mask(None)
            t.render(spp=16, integrator=integrator, frame0=64); t.render(spp=16, integrator=integrator, frame0=80)      # a list with costs
            rebuild.append(timed(t, lambda: t.set_tile_mask(half)))
        say(f"   mask of every 2nd tile + list rebuild, {'costs forgotten' if knob else 'costs carried  '}  {spread(rebuild[2:])}")
    t.debug_set("mask_forgets_costs", 0)
    t.set_tile_mask(None)


def whole_call(t, a, integrator, threshold, truth):
    W, H = a.width, a.height
    res = {}
    runs = [("uniform 64", 64), ("uniform 128", 128), ("uniform 256", 256), ("adaptive", None), ("adaptive, costs forgotten", "forget")]
    for r in range(a.reps + 1):
        for name, what in (runs if r % 2 == 0 else runs[::-1]):
            fresh(t, a.seed)
            t.debug_set("mask_forgets_costs", 1 if what == "forget" else 0)
            if isinstance(what, int):
                ms = timed(t, lambda: t.render(spp=what, integrator=integrator))
                samples, hist = W * H * what, None
            else:
                rep = []
                ms = timed(t, lambda: rep.append(t.render_adaptive(threshold=threshold, max_spp=256, spp=a.first, integrator=integrator)))
                samples = rep[0].samples
                n_t = t.tile_samples().ravel()
                hist = {int(v): int((n_t == v).sum()) for v in np.unique(n_t)}
                hist["passes"] = rep[0].passes; hist["active"] = rep[0].active_tiles; hist["max_error"] = float(rep[0].max_error)
            if r:                                  # the first repetition warms up
                e = res.setdefault(name, dict(ms=[], samples=samples, hist=hist, kernel=[]))
                e["ms"].append(ms); e["kernel"].append(t.stats().kernel_ms)
                if "rmse" not in e:
                    e["rmse"] = rmse(t.download_accum(), truth)
    t.debug_set("mask_forgets_costs", 0)
    for name, _ in runs:
        e = res[name]
        say(f"   {name:26s} wall {spread(e['ms'])}  render kernels {med(e['kernel']):8.3f} ms  {e['samples'] / (W * H):6.1f} spp  RMSE {e['rmse']:.5f}")
        if e["hist"]:
            h = e["hist"]
            say(f"      tiles by n_t: {', '.join(f'{k}: {v}' for k, v in h.items() if isinstance(k, int))}; {h['passes']} passes, {h['active']} tiles "
                f"still active, max E_t {h['max_error']:.4f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--first", type=int, default=16, help="samples of the adaptive call's first pass")
    ap.add_argument("--threshold", type=float, default=None, help="default: what step 0 measures")
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--scenes", default="config2,mesh")
    ap.add_argument("--out", default=None, help="the report goes here too")
    a = ap.parse_args()

    W, H = a.width, a.height
    for which in a.scenes.split(","):
        with Tracer(0) as t:
            if which == "config2":
                sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
                t.upload_scene(sc.view)
                say(f"=== config 2: Cornell box + 12 spheres, {W}x{H}")
            else:
                mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
                if a.copies > 1:
                    mesh = mesh.replicate(a.copies, 1.2)
                sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
                t.upload_scene_device(sc.view, FLAGS)
                say(f"=== Cornell + the replicated ball: {sc.view.n_index // 3} triangles, {W}x{H}")
            t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
            measured = default_threshold(t, a) if which == "config2" else None
            if a.threshold is None:
                a.threshold = measured if measured is not None else t.adaptive_params().threshold
            say(f"   the library's default threshold: {t.adaptive_params().threshold:.5f}; threshold of the runs below: {a.threshold:.5f}, first pass {a.first}")
            for integrator in (abi.INTEGRATOR_MIS, abi.INTEGRATOR_PATH):
                say(f"--- {NAMES[integrator]}")
                say(f"1. per round, medians of {a.reps}")
                per_round(t, a, integrator)
                fresh(t, a.seed + 1000)
                t.render(spp=a.truth_spp, integrator=integrator)
                truth = t.download_accum()
                say(f"2. / 3. the whole call against uniform renders, alternated, medians of {a.reps}; RMSE against {a.truth_spp} spp of another seed")
                whole_call(t, a, integrator, a.threshold, truth)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
