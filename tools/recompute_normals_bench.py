#!/usr/bin/env python3
"""trc_recompute_normals against what a host had before it.

The replicated ball of tools/update_vertices_bench.py (~0.98 M triangles, 49 copies).  Two contexts on the same GPU hold the scene:
  device    every repetition: update_vertices of newly twisted vertices (untimed), then trc_recompute_normals over the whole mesh
  updated   receives the device context's vertices, downloaded (hence the same bits), through update_vertices: the path the call
            replaces -- a host that derives the normals itself uploads 32 B per vertex.  The download and the host's own normal loop
            (numpy here, vectorised over the triangles) come on top of that and are timed apart.
The sides alternate repetition by repetition; medians of --reps warm repetitions of the wall time of the call + synchronize and of the
device time of the call's kernels (trc_debug_refit_ms).  The first repetition's result is compared with the definition
(tests/normals_ref.py) bit for bit: half a million vertices, vertex indices that need three passes of the sort.

The one-off adjacency build is measured on --build-reps fresh contexts: the first call of a scene between two synchronize, less the
device time of that call's own kernels.

The gather's bytes: per vertex 8 B of offsets and 64 B of vertex read and written, per corner 4 B of corner id and the 48 B position
record of its triangle (a record is read once per corner that names it: three times in all, from L2 where the corners are close).  The
record rewrite behind it: per triangle 12 B of indices, three 32 B vertices, 16 B of the old attribute record for the material, and the
48 + 64 B records written.  A wavefront of the gather lasts as long as its longest corner list: `lockstep` is the sum over wavefronts of
64 x the longest list, over the sum of all lists -- 1.0 were every list of a wavefront as long as its longest."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402
from update_vertices_bench import FLAGS, med, spin, vertices_of  # noqa: E402
import normals_ref as nr  # noqa: E402


def host_normals(v, idx):
    """what a host does today: face terms, scattered into the vertices, put on the stored normal's side, normalised (float32, numpy)"""
    tri = idx.reshape(-1, 3)
    c = nr.face_terms(v, idx)
    s = np.zeros((len(v), 3), np.float32)
    for k in range(3):
        np.add.at(s, tri[:, k], c)
    s = np.where(((s * v[:, 3:6]).sum(axis=1) < 0)[:, None], -s, s)
    l = np.sqrt((s * s).sum(axis=1))
    out = v.copy()
    ok = l > 0
    out[ok, 3:6] = s[ok] / l[ok, None]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--build-reps", type=int, default=5)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    a = ap.parse_args()
    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    v0 = vertices_of(sc.view)
    idx = np.ctypeslib.as_array(sc.view.idxList, shape=(sc.view.n_index,)).copy()
    n, n_index, n_tri = len(v0), len(idx), len(idx) // 3
    val = nr.valences(idx, n)
    waves = np.pad(val, (0, -n % 64)).reshape(-1, 64)
    lockstep = 64.0 * waves.max(axis=1).sum() / val.sum()
    adj_bytes = 4 * (n + 1) + 4 * n_index
    gather_bytes = 72 * n + 52 * n_index
    rewrite_bytes = (12 + 96 + 16 + 112) * n_tri
    print(f"scene: {n_tri} triangles, {n} vertices, {n_index} corners; valence min {val.min()} mean {val.mean():.2f} max {val.max()}, "
          f"lockstep {lockstep:.3f}; sort passes {(nr.key_bits(n) + 7) // 8}", flush=True)
    print(f"adjacency kept on the device: {adj_bytes / 1e6:.2f} MB ({adj_bytes} B = 4 (n_vertex + 1) + 4 n_index); temporaries of the build: "
          f"{(16 * n_index) / 1e6:.1f} MB of sort arrays", flush=True)

    def timed(call, t):
        t0 = time.perf_counter(); call(); t.synchronize()
        return (time.perf_counter() - t0) * 1e3, t.refit_ms()

    def line(name, wall, dev=None):
        s = f"   {name:44s}{med(wall):8.3f} ms wall (min {min(wall):.3f}, max {max(wall):.3f})"
        if dev is not None:
            s += f"   {med(dev):8.3f} ms device (min {min(dev):.3f}, max {max(dev):.3f})"
        print(s, flush=True)

    # ---- the one-off build: fresh contexts
    first_wall, first_dev = [], []
    for _ in range(a.build_reps):
        with Tracer(0) as t:
            t.upload_scene_device(sc.view, FLAGS)
            t.synchronize()
            wall, dev = timed(lambda: t.recompute_normals(), t)
            first_wall.append(wall); first_dev.append(dev)
    build = [w - d for w, d in zip(first_wall, first_dev)]
    print(f"first call of a scene, {a.build_reps} fresh contexts:")
    line("recompute_normals (first) + synchronize", first_wall, first_dev)
    print(f"   adjacency build (first call's wall less its kernels' device time): {med(build):.3f} ms (min {min(build):.3f}, max {max(build):.3f})", flush=True)

    with Tracer(0) as device, Tracer(0) as updated:
        for t in (device, updated):
            t.upload_scene_device(sc.view, FLAGS)
        device.update_vertices(v0); device.recompute_normals(); device.synchronize()      # maps, adjacency and pinned staging exist
        updated.update_vertices(v0); updated.synchronize()
        res = {k: ([], []) for k in ("normals", "update")}
        download_ms, loop_ms = [], []
        prev = device.download_vertices()
        for r in range(a.reps):
            moved = spin(v0, 10.0 * (r + 1), twist=True)
            device.update_vertices(moved); device.synchronize()
            sample = {}
            if r % 2:                                                      # the update first: the vertices of the repetition before (as many bytes)
                sample["update"] = timed(lambda: updated.update_vertices(prev), updated)
            sample["normals"] = timed(lambda: device.recompute_normals(), device)
            t0 = time.perf_counter(); got = device.download_vertices(); download_ms.append((time.perf_counter() - t0) * 1e3)
            if r % 2 == 0:
                sample["update"] = timed(lambda: updated.update_vertices(got), updated)
            prev = got
            if r == 0:
                want = nr.recompute(moved, idx)
                bad = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
                print(f"repetition 0 against the definition: {bad} of {n} vertices differ; {len(nr.kept(moved, idx))} keep their bits", flush=True)
                assert bad == 0
            t0 = time.perf_counter(); mine = host_normals(moved, idx); loop_ms.append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                print(f"   the host's loop (another order of summation) lies within {np.abs(mine[:, 3:6] - got[:, 3:6]).max():.2e} of it", flush=True)
            for key, (wall, dev) in sample.items():
                res[key][0].append(wall); res[key][1].append(dev)
        print(f"whole mesh, {n_tri} triangles, medians of {a.reps}:")
        line("recompute_normals + synchronize", *res["normals"])
        line("update_vertices (same vertices) + synchronize", *res["update"])
        line("download_vertices (the host path's way in)", download_ms)
        line("host's normal loop (numpy, float32)", loop_ms)
        nd, ud = med(res["normals"][1]), med(res["update"][1])
        print(f"   wall ratio update / normals {med(res['update'][0]) / med(res['normals'][0]):.2f}x; device {ud:.3f} against {nd:.3f} ms")
        print(f"   bytes host to device: normals 0, update {32 * n}")
        print(f"   bytes moved on the device (estimate): gather {gather_bytes / 1e6:.1f} MB + record rewrite {rewrite_bytes / 1e6:.1f} MB = "
              f"{(gather_bytes + rewrite_bytes) / 1e6:.1f} MB in {nd:.3f} ms: {(gather_bytes + rewrite_bytes) / nd / 1e9:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
