#!/usr/bin/env python3
"""trc_rebuild_tree and trc_tree_cost: what a fresh tree costs from what the device holds, against the only route
there was before it, and what it buys.

The replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, 49 copies), every copy one pose range.  Two motions:
  shuffle   the copies TRANSLATE across one another: copy k goes to the grid position of copy perm[k] (a fresh permutation per
            repetition, always from the rest positions) -- rigid objects travelling through the scene, the case that ruins a refitted tree
  spin      every copy turns in place about its own vertical axis (tools/pose_vertices_bench.py)

  a. trc_rebuild_tree(TRC_TREE_SAH) + synchronize after a shuffle, wall and device time (trc_lbvh_info), against the route without it on
     a second context holding the same posed scene: trc_download_vertices + trc_upload_scene_device(SAH | TRIANGLE_LEAVES) +
     trc_upload_triangle_materials + trc_skin_bind.  The sides alternate repetition by repetition.
  b. trc_tree_cost, wall time.
  c. a 32-spp tracePath launch through the refitted tree against the rebuilt one, with (interior + leaf) / root of each: two contexts
     posed alike, one rebuilt, timed alternately.
Medians of --reps warm repetitions.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, make_poses  # noqa: E402
from pose_vertices_bench import turn_about  # noqa: E402
from update_vertices_bench import FLAGS, med, render_ms, vertices_of  # noqa: E402


def ratio(c):
    return (c.interior_half_area + c.leaf_half_area) / c.root_half_area


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    a = ap.parse_args()
    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    n_copies = a.copies * a.copies
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    v0 = vertices_of(sc.view)
    n, n_tri = len(v0), sc.view.n_index // 3
    per = n // n_copies
    assert per * n_copies == n, "the copies of a replicated mesh hold the same number of vertices each"
    centres = [0.5 * (v0[k * per:(k + 1) * per, :3].astype(np.float64).min(0) + v0[k * per:(k + 1) * per, :3].astype(np.float64).max(0))
               for k in range(n_copies)]
    W, H = a.width, a.height
    print(f"scene: {n_tri} triangles, {n} vertices, {n_copies} copies of {per} vertices, frame {W}x{H}", flush=True)
    eye = np.eye(4, dtype=np.float32)

    def shuffle(seed):
        """copy k translated to where copy perm[k] stands at rest"""
        perm = np.random.default_rng(seed).permutation(n_copies)
        poses = []
        for k in range(n_copies):
            m = eye.copy()
            m[:3, 3] = (centres[perm[k]] - centres[k]).astype(np.float32)
            poses.append((k * per, per, m, eye))
        return make_poses(poses)

    def spin(degrees):
        return make_poses([(k * per, per, *turn_about(centres[k], degrees * (1 + k % 3))) for k in range(n_copies)])

    tri_mat = np.where(np.arange(n_tri) % 2 == 0, 19, 4).astype(np.uint32)
    bones = np.zeros((n, 4), np.int64); bones[:, 0] = np.arange(n) // per
    weights = np.zeros((n, 4), np.float32); weights[:, 0] = 1

    def dress(t, view):
        """an upload and what a host has to put back after it"""
        t.upload_scene_device(view, FLAGS)
        t.upload_triangle_materials(tri_mat)
        t.skin_bind(bones, weights)

    def frame_setup(t):
        t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(1)

    def line(name, xs, unit="ms wall"):
        print(f"   {name:58s}{med(xs):9.3f} {unit} (min {min(xs):.3f}, max {max(xs):.3f})")

    with Tracer(0) as new, Tracer(0) as old:
        # ---- a, b
        for t in (new, old):
            dress(t, sc.view)
            t.pose_vertices(shuffle(100)); t.synchronize()                       # rest copy and maps made, pinned staging warm
        new.rebuild_tree(abi.TREE_SAH); new.synchronize()
        rebuild_wall, rebuild_dev, route_wall, route_dev, cost_wall, worn, fresh = [], [], [], [], [], [], []
        same_tree = True
        for r in range(a.reps):
            poses = shuffle(r)
            new.pose_vertices(poses); new.synchronize()
            dress(old, sc.view); old.pose_vertices(poses); old.synchronize()     # the route forgets the rest copy: from rest again, untimed
            t0 = time.perf_counter(); c = new.tree_cost(); cost_wall.append((time.perf_counter() - t0) * 1e3)
            worn.append(ratio(c))
            t0 = time.perf_counter(); new.rebuild_tree(abi.TREE_SAH); new.synchronize(); rebuild_wall.append((time.perf_counter() - t0) * 1e3)
            rebuild_dev.append(new.lbvh_info()[2])
            fresh.append(ratio(new.tree_cost()))
            t0 = time.perf_counter()
            v = old.download_vertices()
            view = abi.Scene.from_buffer_copy(sc.view); view.triList = C.cast(v.ctypes.data, C.POINTER(abi.TriangleVertex))
            dress(old, view); old.synchronize()
            route_wall.append((time.perf_counter() - t0) * 1e3)
            route_dev.append(old.lbvh_info()[2])
            if r == 0:
                same_tree = bytes(memoryview(new.download_bvh())) == bytes(memoryview(old.download_bvh()))
        print(f"a. a fresh SAH tree after a shuffle of the copies, {n_tri} triangles, medians of {a.reps}:")
        line("rebuild_tree(SAH) + synchronize", rebuild_wall)
        line("   its device time (lbvh_info)", rebuild_dev, "ms device")
        line("download_vertices + upload_scene_device + materials + bind", route_wall)
        line("   the upload's device build time (lbvh_info)", route_dev, "ms device")
        print(f"   wall ratio route / rebuild {med(route_wall) / med(rebuild_wall):.2f}x; the two contexts hold the same tree records: {same_tree}")
        print(f"b. tree_cost, medians of {a.reps}:")
        line("tree_cost", cost_wall)
        print(f"   (interior + leaf) / root: refitted after a shuffle {med(worn):.3f} (min {min(worn):.3f}, max {max(worn):.3f}), "
              f"rebuilt {med(fresh):.3f} (min {min(fresh):.3f}, max {max(fresh):.3f})", flush=True)
        # ---- c
        print(f"c. 32-spp tracePath launch through the refitted tree against the rebuilt one, medians of {a.reps}, the two alternated:")
        for t in (new, old):
            frame_setup(t)
        for name, poses in (("shuffle", shuffle(7)), ("spin 30 degrees", spin(30.0)), ("spin 90 degrees", spin(90.0))):
            for t in (new, old):
                dress(t, sc.view); t.pose_vertices(poses)
            new.rebuild_tree(abi.TREE_SAH)
            costs = {"refitted": ratio(old.tree_cost()), "rebuilt": ratio(new.tree_cost())}
            for t in (new, old):
                for _ in range(3):
                    t.clear_accum(); render_ms(t)
            ms = {"refitted": [], "rebuilt": []}
            for r in range(a.reps):
                for key, t in ((("refitted", old), ("rebuilt", new)) if r % 2 == 0 else (("rebuilt", new), ("refitted", old))):
                    t.clear_accum(); ms[key].append(render_ms(t))
            differ = int((new.download_accum().view(np.uint32) != old.download_accum().view(np.uint32)).any(axis=-1).sum())
            print(f"   {name:16s} refitted {med(ms['refitted']):8.3f} ms (cost {costs['refitted']:.3f}), rebuilt {med(ms['rebuilt']):8.3f} ms "
                  f"(cost {costs['rebuilt']:.3f}): time ratio {med(ms['refitted']) / med(ms['rebuilt']):.3f}, cost ratio "
                  f"{costs['refitted'] / costs['rebuilt']:.3f}; pixels in which the two last frames differ: {differ} of {W * H}", flush=True)
        dress(old, sc.view)
        print(f"   at rest the uploaded tree's cost is {ratio(old.tree_cost()):.3f}")


if __name__ == "__main__":
    main()
