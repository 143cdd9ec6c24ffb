#!/usr/bin/env python3
"""trc_denoise_track_motion: what the switch costs (profiles/r24/denoise_motion.txt).

The replicated ball of tools/pose_vertices_bench.py (~0.98 M triangles) at 1920x1080, every copy turning a little per frame.  Three
contexts on the same GPU hold the same scene and make the same calls, alternating within every repetition:
  off     this build, tracking off (the default)
  on      this build, tracking on: the pose takes the snapshot, trc_denoise writes the motion plane and reprojects through it
  parent  --parent LIB: the library of the commit before, loaded beside this one (it has no switch)
Per repetition and context: trc_pose_vertices + synchronize, one sample per pixel, trc_denoise + synchronize; wall times between two
synchronisations, medians of --reps warm repetitions with their spread.  Per-kernel device times: run the same command under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/denoise_motion_bench.py ...
(k_gbuffer<.., .., MOTION>, k_svgf_temporal<MOTION>, k_snapshot_positions)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tracer_amd import abi, device, host  # noqa: E402
from tracer_amd.device import Tracer, make_poses  # noqa: E402
from pose_vertices_bench import turn_about  # noqa: E402
from update_vertices_bench import FLAGS, med, vertices_of  # noqa: E402

NEW_SYMBOLS = ("trc_denoise_track_motion", "trc_download_motion", "trc_download_history_length", "trc_update_primitives")


class _Absent:
    """stands where the parent library has no such entry point (device._load sets its argtypes); never called"""
    argtypes = restype = None


def parent_tracer(path):
    """a Tracer on another build of the library, beside the in-tree one"""
    real = ctypes.CDLL

    class Older(real):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name in NEW_SYMBOLS:
                    return _Absent()
                raise
    ctypes.CDLL = Older
    try:
        L = device._load(path)
    finally:
        ctypes.CDLL = real
    mine, device._LIB = device._LIB, L
    try:
        return Tracer(0)
    finally:
        device._LIB = mine


def timed(trc, fn):
    trc.synchronize()
    t0 = time.perf_counter()
    fn()
    trc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return f"{med(xs):8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent", default=None, help="libtracer_amd.so of the commit before, for the tracking-off comparison")
    a = ap.parse_args()
    W, H = a.width, a.height
    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    n_copies = a.copies * a.copies
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    v0 = vertices_of(sc.view)
    per = len(v0) // n_copies
    centres = [0.5 * (v0[k * per:(k + 1) * per, :3].astype(np.float64).min(0) + v0[k * per:(k + 1) * per, :3].astype(np.float64).max(0))
               for k in range(n_copies)]
    print(f"scene: {sc.view.n_index // 3} triangles, {len(v0)} vertices, {n_copies} ranges; frame {W}x{H}", flush=True)

    def table(degrees):
        return make_poses([(k * per, per, *turn_about(centres[k], degrees * (1 + k % 3))) for k in range(n_copies)])

    ctxs = {"off": Tracer(0), "on": Tracer(0)}
    if a.parent:
        ctxs["parent"] = parent_tracer(a.parent)
    ctxs["on"].denoise_track_motion(True)
    try:
        for t in ctxs.values():
            t.upload_scene_device(sc.view, FLAGS)
            t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(7)
        pose_ms = {k: [] for k in ctxs}
        denoise_ms = {k: [] for k in ctxs}
        still_ms = {k: [] for k in ctxs}
        for r in range(a.reps + 3):                            # three warm-up repetitions: rest copy, maps, planes, snapshot
            poses = table(0.5 * (r + 1))
            order = list(ctxs) if r % 2 == 0 else list(ctxs)[::-1]
            for name in order:
                t = ctxs[name]
                p = t.denoise_params(demodulate=True)
                dt_pose = timed(t, lambda: t.pose_vertices(poses))
                t.clear_accum(); t.render(spp=1, frame0=r)
                dt = timed(t, lambda: t.denoise(p))
                if name == "on" and r == a.reps + 2:
                    moved = int((t.download_motion()["moved"] == 1).sum())
                dt_still = timed(t, lambda: t.denoise(p))      # nothing moved since: no G-buffer pass, the one-tap temporal pass
                if r >= 3:
                    pose_ms[name].append(dt_pose); denoise_ms[name].append(dt); still_ms[name].append(dt_still)
        hist = {k: float(t.download_history_length().mean()) for k, t in ctxs.items() if k != "parent"}
        print(f"medians of {a.reps} repetitions after 3 warm-up; wall time between two trc_synchronize")
        for name in ctxs:
            print(f"  {name:6s} trc_pose_vertices {spread(pose_ms[name])}   trc_denoise after it {spread(denoise_ms[name])}   "
                  f"trc_denoise again {spread(still_ms[name])}")
        print(f"  tracking on: {moved} of {W * H} pixels moved in the last animated frame; mean history length {hist['on']:.2f} (tracking off: {hist['off']:.2f})")
        print(f"  memory while tracking: snapshot {16 * len(v0) / 2**20:.1f} MiB, motion plane {16 * W * H / 2**20:.1f} MiB")
    finally:
        for t in ctxs.values():
            t.close()


if __name__ == "__main__":
    main()
