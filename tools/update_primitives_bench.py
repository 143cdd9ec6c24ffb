#!/usr/bin/env python3
"""trc_update_primitives against the re-upload it replaces (profiles/r25/update_primitives.txt).

  1. config 2 (Cornell box + 12 spheres, every primitive analytic): the twelve spheres a step further round the box's vertical axis per
     repetition, update_primitives + synchronize against trc_upload_scene of the same scene + synchronize.
  2. Cornell + the replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, device-built SAH tree with triangle leaves): the
     light square, cube 0 and one sphere record replaced, against trc_upload_scene_device of the same scene.
  3. what tracking costs the call: the same update with trc_denoise_track_motion on, a trc_denoise between two calls (every call then takes
     the snapshot: the copy of the primitive section, and of 16 bytes per vertex in scene 2).
The upload side runs on --parent LIB, the library of the commit before, loaded beside this one, where given (else on this build); the
sides alternate within every repetition; wall time between two trc_synchronize, device time of the call's kernels from
trc_debug_refit_ms (per-depth launches and knob refit_single); medians of --reps warm repetitions with their spread.
  4. --quality: RMSE of frame 8 of the orbiting spheres at 160x96, 1 spp per frame, against 2048 spp of the last state, tracked against
     untracked (DESIGN section 10b's figure for analytic primitives)."""
import argparse
import ctypes
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tracer_amd import abi, device, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402
from update_vertices_bench import FLAGS, med  # noqa: E402


class _Absent:
    """stands where the parent library has no such entry point (device._load sets its argtypes); never called"""
    argtypes = restype = None


def parent_tracer(path):
    """a Tracer on another build of the library, beside the in-tree one; entry points it lacks are never called"""
    real = ctypes.CDLL

    class Older(real):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name in abi.DEVICE_SYMBOLS:
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


def lists_of(view):
    sp = (abi.Sphere * view.n_sphere).from_buffer_copy(ctypes.string_at(view.sphereList, ctypes.sizeof(abi.Sphere) * view.n_sphere))
    sq = (abi.Square * view.n_square).from_buffer_copy(ctypes.string_at(view.squareList, ctypes.sizeof(abi.Square) * view.n_square))
    cb = (abi.Cube * view.n_cube).from_buffer_copy(ctypes.string_at(view.cubeList, ctypes.sizeof(abi.Cube) * view.n_cube))
    return sp, sq, cb


def orbit(rest, degrees):
    """the spheres `degrees` further round the vertical axis through (278, *, 278), as examples/trc_render --orbit moves them"""
    a = math.radians(degrees)
    ca, sa = math.cos(a), math.sin(a)
    out = (abi.Sphere * len(rest))()
    for i, s in enumerate(rest):
        x, z = s.center.x - 278.0, s.center.z - 278.0
        out[i] = host.make_sphere(s.radius - 0.0001, (278.0 + ca * x + sa * z, s.center.y, 278.0 - sa * x + ca * z), s.material)
    return out


def timed(trc, fn):
    trc.synchronize()
    t0 = time.perf_counter()
    fn()
    trc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return f"{med(xs):8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def setup(t, W, H):
    t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(7)


def compare(title, sc, upload, change, a, parent):
    """upload(t): the scene's upload on tracer t; change(t, r): repetition r's trc_update_primitives on tracer t"""
    W, H = a.width, a.height
    this, tracked = Tracer(0), Tracer(0)
    other = parent_tracer(parent) if parent else Tracer(0)
    try:
        for t in (this, tracked, other):
            upload(t); setup(t, W, H)
        tracked.denoise_track_motion(True)
        tracked.render(spp=1); tracked.denoise()
        upd, dev_level, dev_single, up, upd_tracked = [], [], [], [], []
        for r in range(a.reps + 3):                                # three warm-up repetitions: maps, staging buffers, snapshot
            order = ("update", "upload") if r % 2 == 0 else ("upload", "update")
            for side in order:
                if side == "update":
                    dt = timed(this, lambda: change(this, r))
                    level = this.refit_ms()
                    this.debug_set("refit_single", 1)
                    change(this, r); single = this.refit_ms()
                    this.debug_set("refit_single", 0)
                    dt_tracked = timed(tracked, lambda: change(tracked, r))
                    tracked.denoise()                              # the next call is the first moving call after a trc_denoise again
                else:
                    dt_up = timed(other, lambda: upload(other))
            if r >= 3:
                upd.append(dt); dev_level.append(level); dev_single.append(single); up.append(dt_up); upd_tracked.append(dt_tracked)
        print(f"{title}, medians of {a.reps} repetitions after 3 warm-up; wall time between two trc_synchronize")
        print(f"   trc_update_primitives                      {spread(upd)}")
        print(f"   ... with tracking on (takes the snapshot)  {spread(upd_tracked)}")
        print(f"   the upload on {'the commit before' if parent else 'this build':18s}           {spread(up)}   ratio {med(up) / med(upd):.1f}x")
        print(f"   the call's kernels, one launch per depth   {spread(dev_level)} device")
        print(f"   the call's kernels, single launch          {spread(dev_single)} device", flush=True)
    finally:
        for t in (this, tracked, other):
            t.close()


def quality(a):
    W, H, n_frames = 160, 96, 8
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    rest = lists_of(sc.view)[0]
    rmse = lambda x, y, sel: float(np.sqrt(np.mean((x[sel][..., :3].astype(np.float64) - y[sel][..., :3].astype(np.float64)) ** 2)))
    outs = {}
    with Tracer(0) as t:
        for on in (True, False):
            t.denoise_track_motion(on)
            t.upload_scene(sc.view); setup(t, W, H); t.seed(5)
            for k in range(n_frames):
                if k:
                    t.update_primitives(spheres=orbit(rest, 3.0 * k))
                t.clear_accum(); t.render(spp=1, frame0=k); t.denoise()
            outs[on] = t.download_denoised()
            if on:
                moved = t.download_motion()["moved"] == 1
                hist = float(t.download_history_length()[moved].mean())
        t.seed(1234); t.clear_accum(); t.render(spp=2048)
        truth = t.download_accum()
    everywhere = np.ones((H, W), bool)
    e = {on: (rmse(outs[on], truth, everywhere), rmse(outs[on], truth, moved)) for on in (True, False)}
    print(f"4. orbiting spheres, 3 degrees per frame, {W}x{H}, 1 spp per frame: RMSE of frame {n_frames} against 2048 spp: tracked {e[True][0]:.5f} "
          f"(moved pixels {e[True][1]:.5f}), untracked {e[False][0]:.5f} (moved pixels {e[False][1]:.5f}); moved pixels {int(moved.sum())}, "
          f"their mean history length {hist:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent", default=None, help="libtracer_amd.so of the commit before, for the upload side")
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()

    sc2 = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    rest2 = lists_of(sc2.view)[0]
    compare("1. config 2: the 12 spheres", sc2, lambda t: t.upload_scene(sc2.view),
            lambda t, r: t.update_primitives(spheres=orbit(rest2, 2.0 * (r + 1))), a, a.parent)

    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    sp, sq, cb = lists_of(sc.view)

    def change(t, r):
        s = sq[5]
        light = host.make_square(s.axis_i, s.range_i.x - 2.0 * (r + 1), s.range_i.y - 2.0 * (r + 1), s.axis_j, s.range_j.x, s.range_j.y, s.axis_k, s.value_k, s.material)
        a_ = math.radians(15.0 + r)
        ca, sa = math.cos(a_), math.sin(a_)
        model = np.array([[ca * 165, 0, sa * 165, 265], [0, 330, 0, 1], [-sa * 165, 0, ca * 165, 295], [0, 0, 0, 1]], np.float32)
        t.update_primitives(spheres=orbit(sp[:1], r + 1.0), squares=[light], first_square=5, cubes=[host.make_cube(cb[0].material, model)])
    print(f"scene 2: {sc.view.n_index // 3} triangles, {sc.view.n_vertex} vertices", flush=True)
    compare("2. Cornell + the replicated ball: the light square, cube 0, one sphere record", sc, lambda t: t.upload_scene_device(sc.view, FLAGS), change, a, a.parent)
    if a.quality:
        quality(a)


if __name__ == "__main__":
    main()
