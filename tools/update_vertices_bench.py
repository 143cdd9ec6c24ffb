#!/usr/bin/env python3
"""trc_update_vertices against the re-upload it replaces.

  1. a frame's geometry change on a replicated ball of ~1.0 M triangles: wall time of update_vertices (all vertices) + synchronize
     against trc_upload_scene_device(SAH | TRIANGLE_LEAVES) of the same scene; device time of the update's kernels, per-level and
     single-launch (knob refit_single).  The two sides alternate in one session; medians of --reps warm repetitions.
  2. the first 32-spp launch after the change under a 1 degree per frame spin: costs kept (update) against costs forgotten (re-upload).
  3. ms per launch through the refitted tree against a freshly built SAH tree of the same twisted mesh, at 5 / 30 / 90 degrees.
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402

FLAGS = abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES


def vertices_of(view):
    a = (C.c_float * (8 * view.n_vertex)).from_address(C.addressof(view.triList.contents))
    return np.frombuffer(a, dtype=np.float32).reshape(-1, 8).copy()


def spin(v, degrees, twist=False):
    """the mesh turned about the vertical axis through its box centre; twist: by -degrees / 2 at the bottom to +degrees / 2 at the top"""
    a = math.radians(degrees)
    out = v.astype(np.float64)
    lo, hi = out[:, :3].min(0), out[:, :3].max(0)
    c = 0.5 * (lo + hi)
    q = out[:, :3] - c
    if twist:
        a = a * q[:, 1] / max(hi[1] - lo[1], 1e-9)
    ca, sa = np.cos(a), np.sin(a)
    out[:, 0] = c[0] + ca * q[:, 0] + sa * q[:, 2]; out[:, 2] = c[2] - sa * q[:, 0] + ca * q[:, 2]
    n = out[:, 3:6].copy()
    out[:, 3] = ca * n[:, 0] + sa * n[:, 2]; out[:, 5] = -sa * n[:, 0] + ca * n[:, 2]
    return out.astype(np.float32)


def med(xs):
    return float(np.median(xs))


def render_ms(t, spp=32):
    t.synchronize(); t.reset_stats()
    t0 = time.perf_counter()
    t.render(spp=spp, integrator=abi.INTEGRATOR_PATH)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    a = ap.parse_args()
    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    v0 = vertices_of(sc.view)
    n_tri = sc.view.n_index // 3
    print(f"scene: {n_tri} triangles, {len(v0)} vertices, frame {a.width}x{a.height}", flush=True)
    W, H = a.width, a.height
    with Tracer(0) as t:
        t.upload_scene_device(sc.view, FLAGS)
        t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(1)
        # ---- 1
        t.update_vertices(v0); t.synchronize()                                  # maps made, pinned staging warm
        upd, up, dev_level, dev_single = [], [], [], []
        for r in range(a.reps):
            v = spin(v0, r + 1.0)
            t0 = time.perf_counter(); t.update_vertices(v); t.synchronize(); upd.append((time.perf_counter() - t0) * 1e3)
            dev_level.append(t.refit_ms())
            t.debug_set("refit_single", 1)
            t.update_vertices(v); t.synchronize(); dev_single.append(t.refit_ms())
            t.debug_set("refit_single", 0)
            view = abi.Scene.from_buffer_copy(sc.view)
            view.triList = C.cast(v.ctypes.data, C.POINTER(abi.TriangleVertex))
            t0 = time.perf_counter(); t.upload_scene_device(view, FLAGS); t.synchronize(); up.append((time.perf_counter() - t0) * 1e3)
            t.update_vertices(v); t.synchronize()                               # the maps of the new blob, outside the timed part
        print(f"1. geometry change, {n_tri} triangles, medians of {a.reps}:")
        print(f"   update_vertices + synchronize      {med(upd):8.3f} ms wall   (min {min(upd):.3f}, max {max(upd):.3f})")
        print(f"   upload_scene_device + synchronize  {med(up):8.3f} ms wall   (min {min(up):.3f}, max {max(up):.3f})   ratio {med(up) / med(upd):.2f}x")
        print(f"   update kernels, one launch per depth {med(dev_level):8.3f} ms device (min {min(dev_level):.3f}, max {max(dev_level):.3f})")
        print(f"   update kernels, single launch        {med(dev_single):8.3f} ms device (min {min(dev_single):.3f}, max {max(dev_single):.3f})")
        print(f"   bytes: {32 * len(v0) / 1e6:.1f} MB of vertices H2D on both sides; the update rewrites {112 * n_tri / 1e6:.1f} MB of records and {64 * (n_tri + 12) / 1e6:.1f} MB of nodes", flush=True)
        # ---- 2
        kept, forgot, settled = [], [], []
        t.upload_scene_device(sc.view, FLAGS)
        for _ in range(4):
            t.clear_accum(); render_ms(t)
        for r in range(a.reps):
            v = spin(v0, r + 1.0)
            t.update_vertices(v); t.clear_accum(); kept.append(render_ms(t))
            t.clear_accum(); settled.append(render_ms(t))
        for r in range(a.reps):
            v = spin(v0, r + 1.0)
            view = abi.Scene.from_buffer_copy(sc.view); view.triList = C.cast(v.ctypes.data, C.POINTER(abi.TriangleVertex))
            t.upload_scene_device(view, FLAGS); t.clear_accum(); forgot.append(render_ms(t))
        print(f"2. first 32-spp launch after a 1 degree spin, medians of {a.reps}:")
        print(f"   after update_vertices (costs kept)          {med(kept):8.3f} ms")
        print(f"   after upload_scene_device (costs forgotten) {med(forgot):8.3f} ms")
        print(f"   second launch after the update (settled)    {med(settled):8.3f} ms", flush=True)
        # ---- 3
        print(f"3. 32-spp launch through the refitted tree against a fresh SAH tree of the same mesh, medians of {a.reps}:")
        for deg in (5, 30, 90):
            v = spin(v0, deg, twist=True)
            t.upload_scene_device(sc.view, FLAGS); t.update_vertices(v)
            for _ in range(3):
                t.clear_accum(); render_ms(t)
            refit = [(t.clear_accum(), render_ms(t))[1] for _ in range(a.reps)]
            view = abi.Scene.from_buffer_copy(sc.view); view.triList = C.cast(v.ctypes.data, C.POINTER(abi.TriangleVertex))
            t.upload_scene_device(view, FLAGS)
            for _ in range(3):
                t.clear_accum(); render_ms(t)
            fresh = [(t.clear_accum(), render_ms(t))[1] for _ in range(a.reps)]
            print(f"   twist {deg:3d} degrees: refitted {med(refit):8.3f} ms, fresh {med(fresh):8.3f} ms, ratio {med(refit) / med(fresh):.3f}", flush=True)


if __name__ == "__main__":
    main()
