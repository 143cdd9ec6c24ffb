#!/usr/bin/env python3
"""trc_morph_vertices, alone and with the skin on top, against what a host had before it.

The replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, 49 copies) with the bones of tools/skin_vertices_bench.py
(four per copy, 196 in all).  64 targets are bound over every vertex (24 B per vertex and target: 0.77 GB of device memory), of which a
frame gives 4 or 32 a weight that is not zero.  Four contexts on the same GPU hold the same scene:
  morphed   morph binding + skin binding: trc_morph_vertices, morph only and fused
  updated   receives the morphed context's final vertices through update_vertices (downloaded, hence the same bits)
  skinned   skin binding: trc_skin_vertices alone
  pair      skin binding: trc_skin_vertices and then update_vertices of the morph's range with the fused call's final vertices -- how a
            host reached skin(rest + morph) before (and the update overwrites the rest copy of that range, so it is a full vertex
            upload per frame in practice; the timing is the same)
The sides alternate repetition by repetition; medians of --reps warm repetitions of the wall time of the call(s) + synchronize and of
the device time of the call's kernels (trc_debug_refit_ms).  The morph kernel's own time is the device time of the morph less the device
time of the update of the same vertices -- the same record rewrite and refit chain without a kernel in front -- and its achieved
bandwidth is its byte count, 64 + 24 * A bytes per vertex (32 read of the rest copy, 32 written, 24 per active target), over that.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, make_bones  # noqa: E402
from pose_vertices_bench import turn_about  # noqa: E402
from update_vertices_bench import FLAGS, med, vertices_of  # noqa: E402

BONES_PER_COPY = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--active", type=int, nargs="+", default=[4, 32])
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
    print(f"scene: {n_tri} triangles, {n} vertices, {n_bones} bones, {a.targets} targets bound over every vertex "
          f"({24 * a.targets * n / 1e6:.0f} MB of deltas)", flush=True)

    rng = np.random.default_rng(3)
    bones = (np.arange(n)[:, None] // per) * BONES_PER_COPY + rng.permuted(np.tile(np.arange(BONES_PER_COPY), (n, 1)), axis=1)
    skin_w = (rng.random((n, 4)) + 0.1).astype(np.float32)
    skin_w /= skin_w.sum(axis=1, keepdims=True)
    deltas = rng.random((a.targets, n, 6), dtype=np.float32)
    deltas -= np.float32(0.5)

    def palette(degrees):
        return make_bones([turn_about(centres[k], 0.5 * degrees * (1 + (k + j) % 3)) for k in range(n_copies) for j in range(BONES_PER_COPY)])

    def weights(n_active, r):
        """n_active weights that are not zero, spread evenly over the targets, another set of values every repetition"""
        w = np.zeros(a.targets, np.float32)
        k = (np.arange(n_active) * a.targets) // n_active
        w[k] = (0.2 + 0.6 * ((np.arange(n_active) * 0.618 + 0.37 * r) % 1.0)).astype(np.float32)
        assert np.count_nonzero(w) == n_active
        return w

    def timed(call, t):
        t0 = time.perf_counter(); call(); t.synchronize()
        return (time.perf_counter() - t0) * 1e3, t.refit_ms()

    def line(name, wall, dev=None):
        s = f"   {name:44s}{med(wall):8.3f} ms wall (min {min(wall):.3f}, max {max(wall):.3f})"
        if dev is not None:
            s += f"   {med(dev):8.3f} ms device (min {min(dev):.3f}, max {max(dev):.3f})"
        print(s)

    with Tracer(0) as morphed, Tracer(0) as updated, Tracer(0) as skinned, Tracer(0) as pair:
        for t in (morphed, updated, skinned, pair):
            t.upload_scene_device(sc.view, FLAGS)
        morphed.morph_bind(deltas)
        for t in (morphed, skinned, pair):
            t.skin_bind(bones, skin_w)
        # rest copies and maps made, pinned staging warm, both kernels of the morphed context run once
        morphed.morph_vertices(weights(4, 0)); morphed.morph_vertices(weights(4, 0), palette(0.5)); morphed.synchronize()
        updated.update_vertices(v0); updated.synchronize()
        skinned.skin_vertices(palette(0.5)); skinned.synchronize()
        pair.skin_vertices(palette(0.5)); pair.update_vertices(v0); pair.synchronize()
        for n_active in a.active:
            keys = ("morph", "update", "skin", "fused", "pair")
            res = {k: ([], []) for k in keys}
            for r in range(a.reps):
                w, pal = weights(n_active, r), palette(r + 1.0)
                sample = {"morph": timed(lambda: morphed.morph_vertices(w), morphed)}
                assert morphed.pose_overflows() == 0
                v = morphed.download_vertices()                                 # the same final vertices, bit for bit
                sample["update"] = timed(lambda: updated.update_vertices(v), updated)
                assert np.array_equal(updated.download_vertices().view(np.uint32), v.view(np.uint32))
                sample["skin"] = timed(lambda: skinned.skin_vertices(pal), skinned)
                sample["fused"] = timed(lambda: morphed.morph_vertices(w, pal), morphed)
                vf = morphed.download_vertices()

                def skin_then_update():
                    pair.skin_vertices(pal)
                    pair.update_vertices(vf)
                sample["pair"] = timed(skin_then_update, pair)
                assert np.array_equal(pair.download_vertices().view(np.uint32), vf.view(np.uint32))
                pair.update_vertices(v0)                                        # the rest copy back to what the others skin from
                for key, (wall, dev) in sample.items():
                    res[key][0].append(wall); res[key][1].append(dev)
            print(f"{n_active} active targets of {a.targets}, one launch per depth, {n_tri} triangles, medians of {a.reps}:")
            line("morph_vertices + synchronize", *res["morph"])
            line("update_vertices (same bits) + synchronize", *res["update"])
            line("skin_vertices + synchronize", *res["skin"])
            line("morph_vertices with bones + synchronize", *res["fused"])
            line("skin_vertices, update_vertices + synchronize", res["pair"][0])
            kernel_ms = med(res["morph"][1]) - med(res["update"][1])
            kernel_bytes = (64 + 24 * n_active) * n
            spread = max(res["update"][1]) - min(res["update"][1])                # of the chain alone: what the difference must pass to mean anything
            bandwidth = f"{kernel_bytes / kernel_ms / 1e9:.2f} TB/s" if kernel_ms > spread else f"not resolved (the chain's own spread is {spread:.3f} ms)"
            print(f"   wall ratio update / morph {med(res['update'][0]) / med(res['morph'][0]):.2f}x, morph / skin {med(res['morph'][0]) / med(res['skin'][0]):.2f}x, "
                  f"pair / fused {med(res['pair'][0]) / med(res['fused'][0]):.2f}x")
            print(f"   bytes host to device: morph {8 * n_active}, fused {8 * n_active + 128 * n_bones}, skin {128 * n_bones}, update {32 * n}, "
                  f"pair {128 * n_bones + 32 * n}")
            print(f"   morph kernel alone (device, morph - update): {kernel_ms:.3f} ms for {kernel_bytes / 1e6:.1f} MB ({64 + 24 * n_active} B per vertex): {bandwidth}",
                  flush=True)


if __name__ == "__main__":
    main()
