#!/usr/bin/env python3
"""TRC_TREE_SAH3 against TRC_TREE_SAH: what the three-axis, 32-bin split costs to build and what it buys per ray.

Both flavours in one process on one GPU, one context each, the sides alternating repetition by repetition; medians of --reps warm
repetitions with their spread.  The TRC_TREE_SAH side is the baseline: its kernels and its tree are the parent commit's (the flag adds
kernels, it changes none of them), so it is never the flagged build against itself.

Scenes:
  config3   Cornell + coatball.obj, traceMIS                          (BASELINE config 3 as named)
  config4   Cornell + teapot.obj x 64, tracePath                      (BASELINE config 4 as named)
  shuffle49 the 49-copy ball of tools/rebuild_tree_bench.py after the copies have traded places (pose_vertices), tracePath: the tree is
            a REBUILD with the flavour's flag
  teapot256 teapot.obj x 256 = 4.0 M triangles, tracePath             (--big)
Per scene and flavour: upload (trc_upload_scene_device with TRC_TREE_TRIANGLE_LEAVES) and rebuild (trc_rebuild_tree), wall and device
ms; tree height; (interior + leaf) / root and interior / root of trc_tree_cost; N_descend and N_return per ray of a TRC_FLAG_COLLECT_STATS
launch; ms of a 32-spp launch at 1920 x 1080.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, make_poses  # noqa: E402
from update_vertices_bench import med, vertices_of  # noqa: E402

FLAVOURS = {"sah": abi.TREE_SAH, "sah3": abi.TREE_SAH | abi.TREE_SAH3}


def spread(xs):
    return f"{med(xs):9.3f} (min {min(xs):.3f}, max {max(xs):.3f})"


def launch_ms(t, integrator, spp=32):
    t.synchronize()
    t0 = time.perf_counter()
    t.render(spp=spp, integrator=integrator)
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def scenes(big):
    out = [("config3", host.Mesh.golden("coatball"), abi.INTEGRATOR_MIS, None),
           ("config4", host.Mesh.golden("teapot").replicate(8, 80.0), abi.INTEGRATOR_PATH, None),
           ("shuffle49", host.Mesh.ball(100, 100, 0.08).replicate(7, 1.2), abi.INTEGRATOR_PATH, 49)]
    if big:
        out.append(("teapot256", host.Mesh.golden("teapot").replicate(16, 80.0), abi.INTEGRATOR_PATH, None))
    return out


def shuffle_poses(v0, n_copies, seed):
    per = len(v0) // n_copies
    centres = [0.5 * (v0[k * per:(k + 1) * per, :3].astype(np.float64).min(0) + v0[k * per:(k + 1) * per, :3].astype(np.float64).max(0))
               for k in range(n_copies)]
    perm = np.random.default_rng(seed).permutation(n_copies)
    eye = np.eye(4, dtype=np.float32)
    poses = []
    for k in range(n_copies):
        m = eye.copy()
        m[:3, 3] = (centres[perm[k]] - centres[k]).astype(np.float32)
        poses.append((k * per, per, m, eye))
    return make_poses(poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    W, H = a.width, a.height
    for name, mesh, integrator, n_copies in scenes(a.big):
        if a.only and name not in a.only.split(","):
            continue
        sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
        n_tri = sc.view.n_index // 3
        print(f"{name}: {n_tri} triangles, {'traceMIS' if integrator == abi.INTEGRATOR_MIS else 'tracePath'}, frame {W}x{H}, medians of {a.reps}", flush=True)
        with Tracer(0) as t_sah, Tracer(0) as t_sah3:
            ctx = {"sah": t_sah, "sah3": t_sah3}
            up_wall, up_dev, re_wall, re_dev, ms = ({k: [] for k in FLAVOURS} for _ in range(5))
            poses = shuffle_poses(vertices_of(sc.view), n_copies, 7) if n_copies else None

            def build(k, timed):
                t, flags = ctx[k], FLAVOURS[k]
                t.synchronize()
                t0 = time.perf_counter(); t.upload_scene_device(sc.view, flags | abi.TREE_TRIANGLE_LEAVES); t.synchronize()
                if timed:
                    up_wall[k].append((time.perf_counter() - t0) * 1e3); up_dev[k].append(t.lbvh_info()[2])
                if poses is not None:
                    t.pose_vertices(poses); t.synchronize()
                t0 = time.perf_counter(); t.rebuild_tree(flags); t.synchronize()
                if timed:
                    re_wall[k].append((time.perf_counter() - t0) * 1e3); re_dev[k].append(t.lbvh_info()[2])

            for k in FLAVOURS:                                  # warm: allocator, pinned staging, code objects
                build(k, False)
            for r in range(a.reps):
                for k in (("sah", "sah3") if r % 2 == 0 else ("sah3", "sah")):
                    build(k, True)
            info = {}
            for k, t in ctx.items():
                t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(1)
                c = t.tree_cost()
                t.clear_accum(); t.reset_stats(); t.render(spp=1, integrator=integrator, collect_stats=True); t.synchronize()
                st = t.stats()
                info[k] = dict(height=t.lbvh_info()[1], ratio=(c.interior_half_area + c.leaf_half_area) / c.root_half_area,
                               interior=c.interior_half_area / c.root_half_area, descend=st.n_descend / st.rays, ret=st.n_return / st.rays, rays=st.rays)
                for _ in range(3):
                    t.clear_accum(); launch_ms(t, integrator)
            for r in range(a.reps):
                for k in (("sah", "sah3") if r % 2 == 0 else ("sah3", "sah")):
                    ctx[k].clear_accum(); ms[k].append(launch_ms(ctx[k], integrator))
            same = int((t_sah.download_accum().view(np.uint32) != t_sah3.download_accum().view(np.uint32)).any(axis=-1).sum())
            for k in FLAVOURS:
                i = info[k]
                print(f"  {k:5s} upload wall {spread(up_wall[k])} ms, device {spread(up_dev[k])} ms")
                print(f"        rebuild wall {spread(re_wall[k])} ms, device {spread(re_dev[k])} ms")
                print(f"        height {i['height']}, (interior + leaf) / root {i['ratio']:.3f}, interior / root {i['interior']:.3f}, "
                      f"N_descend / ray {i['descend']:.3f}, N_return / ray {i['ret']:.3f} ({i['rays']} rays)")
                print(f"        32-spp launch {spread(ms[k])} ms")
            print(f"  sah3 / sah: upload device {med(up_dev['sah3']) / med(up_dev['sah']):.3f}, rebuild device {med(re_dev['sah3']) / med(re_dev['sah']):.3f}, "
                  f"interior / root {info['sah3']['interior'] / info['sah']['interior']:.4f}, N_descend {info['sah3']['descend'] / info['sah']['descend']:.4f}, "
                  f"launch {med(ms['sah3']) / med(ms['sah']):.4f}; pixels in which the two last frames differ: {same} of {W * H}", flush=True)


if __name__ == "__main__":
    main()
