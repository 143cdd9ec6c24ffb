#!/usr/bin/env python3
"""trc_pose_vertices against the trc_update_vertices it replaces for rigid motion.

The replicated ball of tools/update_vertices_bench.py (~0.98 M triangles), every copy one range turning about the vertical axis through
its own box centre.  Two contexts on the same GPU hold the same scene: one is posed (144 bytes per copy cross the bus), the other
receives the same final vertices through update_vertices (32 bytes per vertex).  The two sides alternate within the session; medians of
--reps warm repetitions of
  - wall time of the call + synchronize
  - device time of the call's kernels (trc_debug_refit_ms: the pose kernel is inside the pose's figure)
for both refit variants (knob refit_single).
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, make_poses  # noqa: E402
from update_vertices_bench import FLAGS, med, vertices_of  # noqa: E402


def turn_about(centre, degrees):
    """T(c) * R_y(a) * T(-c) as a (4, 4) float32 matrix, and the rotation alone for the normals"""
    a = math.radians(degrees)
    ca, sa = math.cos(a), math.sin(a)
    rot = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1]], dtype=np.float64)
    model = rot.copy()
    model[:3, 3] = centre - rot[:3, :3] @ centre
    return model.astype(np.float32), rot.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    a = ap.parse_args()
    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    n_copies = a.copies * a.copies
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    v0 = vertices_of(sc.view)
    n_tri = sc.view.n_index // 3
    per = len(v0) // n_copies
    assert per * n_copies == len(v0), "the copies of a replicated mesh hold the same number of vertices each"
    centres = [0.5 * (v0[k * per:(k + 1) * per, :3].astype(np.float64).min(0) + v0[k * per:(k + 1) * per, :3].astype(np.float64).max(0))
               for k in range(n_copies)]
    print(f"scene: {n_tri} triangles, {len(v0)} vertices, {n_copies} ranges of {per} vertices", flush=True)

    def table(degrees):
        return make_poses([(k * per, per, *turn_about(centres[k], degrees * (1 + k % 3))) for k in range(n_copies)])

    with Tracer(0) as posed, Tracer(0) as updated:
        for t in (posed, updated):
            t.upload_scene_device(sc.view, FLAGS)
        posed.pose_vertices(table(0.5)); posed.synchronize()                     # rest copy and maps made, pinned staging warm
        updated.update_vertices(v0); updated.synchronize()
        for single in (0, 1):
            posed.debug_set("refit_single", single); updated.debug_set("refit_single", single)
            pose_wall, pose_dev, upd_wall, upd_dev = [], [], [], []
            for r in range(a.reps):
                poses = table(r + 1.0)
                t0 = time.perf_counter(); posed.pose_vertices(poses); posed.synchronize(); pose_wall.append((time.perf_counter() - t0) * 1e3)
                pose_dev.append(posed.refit_ms())
                assert posed.pose_overflows() == 0
                v = posed.download_vertices()                                    # the same final vertices, bit for bit
                t0 = time.perf_counter(); updated.update_vertices(v); updated.synchronize(); upd_wall.append((time.perf_counter() - t0) * 1e3)
                upd_dev.append(updated.refit_ms())
            name = "single launch" if single else "one launch per depth"
            print(f"refit: {name}, {n_tri} triangles, medians of {a.reps}:")
            print(f"   pose_vertices + synchronize    {med(pose_wall):8.3f} ms wall (min {min(pose_wall):.3f}, max {max(pose_wall):.3f})   "
                  f"{med(pose_dev):8.3f} ms device (min {min(pose_dev):.3f}, max {max(pose_dev):.3f})")
            print(f"   update_vertices + synchronize  {med(upd_wall):8.3f} ms wall (min {min(upd_wall):.3f}, max {max(upd_wall):.3f})   "
                  f"{med(upd_dev):8.3f} ms device (min {min(upd_dev):.3f}, max {max(upd_dev):.3f})")
            print(f"   wall ratio update / pose {med(upd_wall) / med(pose_wall):.2f}x; bytes host to device: {144 * n_copies} against {32 * len(v0)}", flush=True)
        same = np.array_equal(posed.download_vertices().view(np.uint32), updated.download_vertices().view(np.uint32))
        print(f"the two contexts hold the same vertices: {same}")


if __name__ == "__main__":
    main()
