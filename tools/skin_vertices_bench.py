#!/usr/bin/env python3
"""trc_skin_vertices against the trc_update_vertices it replaces for geometry that bends, and against trc_pose_vertices
(DESIGN section 4.13).

The replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, 49 copies).  Every copy has four bones of its own (196 in
all: turns of different angles about the vertical axis through the copy's box centre) and every vertex four non-zero weights.  Three
contexts on the same GPU hold the same scene: one is skinned (128 bytes per bone cross the bus), one receives the same final vertices
through update_vertices (32 bytes per vertex; downloaded from the skinned context, hence the same bits), one is posed with 49 rigid
ranges.  The sides alternate repetition by repetition; medians of --reps warm repetitions of
  - wall time of the call + synchronize
  - device time of the call's kernels (trc_debug_refit_ms: the skin kernel is inside the skin's figure)
and then the staged palette (LDS) against the gathered one (knob skin_no_lds), alternated likewise, at 196 bones and at
abi.SKIN_LDS_BONES (the palette padded with bones that no vertex names: the staged kernel loads them all the same).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, make_bones, make_poses  # noqa: E402
from pose_vertices_bench import turn_about  # noqa: E402
from update_vertices_bench import FLAGS, med, vertices_of  # noqa: E402

BONES_PER_COPY = 4


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
    n, n_tri = len(v0), sc.view.n_index // 3
    per = n // n_copies
    assert per * n_copies == n, "the copies of a replicated mesh hold the same number of vertices each"
    centres = [0.5 * (v0[k * per:(k + 1) * per, :3].astype(np.float64).min(0) + v0[k * per:(k + 1) * per, :3].astype(np.float64).max(0))
               for k in range(n_copies)]
    n_bones = BONES_PER_COPY * n_copies
    print(f"scene: {n_tri} triangles, {n} vertices, {n_copies} copies of {per} vertices, {n_bones} bones", flush=True)

    rng = np.random.default_rng(3)
    bones = (np.arange(n)[:, None] // per) * BONES_PER_COPY + rng.permuted(np.tile(np.arange(BONES_PER_COPY), (n, 1)), axis=1)
    weights = (rng.random((n, 4)) + 0.1).astype(np.float32)
    weights /= weights.sum(axis=1, keepdims=True)
    assert (weights != 0).all() and bones.max() == n_bones - 1

    def palette(degrees, size=n_bones):
        """bone j of copy k turns by degrees * (1 + (k + j) % 3) / 2 about the copy's axis; padded to `size` bones with the last one"""
        pal = [turn_about(centres[k], 0.5 * degrees * (1 + (k + j) % 3)) for k in range(n_copies) for j in range(BONES_PER_COPY)]
        return make_bones(pal + [pal[-1]] * (size - len(pal)))

    def table(degrees):
        return make_poses([(k * per, per, *turn_about(centres[k], degrees * (1 + k % 3))) for k in range(n_copies)])

    def timed(call, t):
        t0 = time.perf_counter(); call(); t.synchronize()
        return (time.perf_counter() - t0) * 1e3, t.refit_ms()

    def line(name, wall, dev):
        print(f"   {name:32s}{med(wall):8.3f} ms wall (min {min(wall):.3f}, max {max(wall):.3f})   "
              f"{med(dev):8.3f} ms device (min {min(dev):.3f}, max {max(dev):.3f})")

    with Tracer(0) as skinned, Tracer(0) as updated, Tracer(0) as posed:
        for t in (skinned, updated, posed):
            t.upload_scene_device(sc.view, FLAGS)
        skinned.skin_bind(bones, weights)
        skinned.skin_vertices(palette(0.5)); skinned.synchronize()              # rest copy and maps made, pinned staging warm
        updated.update_vertices(v0); updated.synchronize()
        posed.pose_vertices(table(0.5)); posed.synchronize()
        res = {k: ([], []) for k in ("skin", "update", "pose")}
        for r in range(a.reps):
            pal, poses = palette(r + 1.0), table(r + 1.0)
            sample = {"skin": timed(lambda: skinned.skin_vertices(pal), skinned)}
            assert skinned.pose_overflows() == 0
            v = skinned.download_vertices()                                     # the same final vertices, bit for bit
            sample["update"] = timed(lambda: updated.update_vertices(v), updated)
            sample["pose"] = timed(lambda: posed.pose_vertices(poses), posed)
            for key, (wall, dev) in sample.items():
                res[key][0].append(wall); res[key][1].append(dev)
        print(f"one launch per depth, {n_tri} triangles, medians of {a.reps}:")
        line("skin_vertices + synchronize", *res["skin"])
        line("update_vertices + synchronize", *res["update"])
        line("pose_vertices + synchronize", *res["pose"])
        print(f"   wall ratio update / skin {med(res['update'][0]) / med(res['skin'][0]):.2f}x, skin / pose {med(res['skin'][0]) / med(res['pose'][0]):.2f}x; "
              f"bytes host to device: skin {128 * n_bones}, pose {144 * n_copies}, update {32 * n}", flush=True)
        same = np.array_equal(skinned.download_vertices().view(np.uint32), updated.download_vertices().view(np.uint32))
        print(f"the skinned and the updated context hold the same vertices: {same}")
        # the two palette paths of the kernel
        for size in (n_bones, abi.SKIN_LDS_BONES):
            if size < n_bones or size > abi.SKIN_LDS_BONES:
                print(f"palette of {size} bones: not staged (SKIN_LDS_BONES = {abi.SKIN_LDS_BONES}), nothing to compare")
                continue
            res = {0: ([], []), 1: ([], [])}
            bits = {}
            for r in range(a.reps):
                pal = palette(r + 1.0, size)
                for knob in ((0, 1) if r % 2 == 0 else (1, 0)):
                    skinned.debug_set("skin_no_lds", knob)
                    wall, dev = timed(lambda: skinned.skin_vertices(pal), skinned)
                    res[knob][0].append(wall); res[knob][1].append(dev)
                    bits[knob] = skinned.download_vertices().view(np.uint32)
                assert np.array_equal(bits[0], bits[1])
            skinned.debug_set("skin_no_lds", 0)
            print(f"palette of {size} bones, medians of {a.reps} (the device time is the skin kernel + the refit chain):")
            line("staged in LDS", *res[0])
            line("gathered from memory", *res[1])


if __name__ == "__main__":
    main()
