#!/usr/bin/env python3
"""trc_set_triangle_visibility: what showing and hiding objects costs from what the device holds, against a plain
rebuild and against the only route there was before it.

The replicated ball of tools/rebuild_tree_bench.py (~0.98 M triangles, 49 copies; an object = one copy's triangles, one range).

  a. trc_rebuild_tree(TRC_TREE_SAH) and trc_rebuild_tree(0) + synchronize: the yardstick, with its run-to-run spread.
  b. trc_set_triangle_visibility(TRC_TREE_SAH) + synchronize with nothing hidden, one object hidden, half the objects hidden and all shown
     again (each from the state the line names: the call in front of it, untimed, puts the scene there); wall time, the call's device time
     (trc_lbvh_info) and the device time of its leaf-list stage alone -- mask, partition, leaf records (trc_debug_visibility_ms).  The
     nothing-hidden case under the LBVH too.
  c. the route without the call, on a second context: trc_download_vertices + trc_upload_scene_device(SAH | TRIANGLE_LEAVES) of the index
     list without the hidden objects' triangles, for the same three subsets.
One warm-up of every timed call, then medians of --reps repetitions with minimum and maximum; a, b and c alternate repetition by
repetition.  --out: the report goes there as well as to the terminal.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402
from update_vertices_bench import FLAGS, med, vertices_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ball", type=int, default=100)          # 2 * 100 * 100 = 20 000 triangles ...
    ap.add_argument("--copies", type=int, default=7)          # ... x 7 x 7 = 0.98 M
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    mesh = host.Mesh.ball(a.ball, a.ball, 0.08)
    n_copies = a.copies * a.copies
    if a.copies > 1:
        mesh = mesh.replicate(a.copies, 1.2)
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=True)
    n_tri = sc.view.n_index // 3
    per = n_tri // n_copies
    assert per * n_copies == n_tri, "the copies of a replicated mesh hold the same number of triangles each"
    idx = np.frombuffer((C.c_uint32 * sc.view.n_index).from_address(C.addressof(sc.view.idxList.contents)), dtype=np.uint32).copy()
    say(f"scene: {n_tri} triangles, {len(vertices_of(sc.view))} vertices, {n_copies} objects of {per} triangles")
    everything = [(0, n_tri, 1)]
    subsets = {"nothing hidden": [], "one object hidden": [(3 * per, per, 0)],
               "half the objects hidden": [(k * per, per, 0) for k in range(0, n_copies, 2)]}

    def subset_view(ranges, vertices):
        keep = np.ones(n_tri, bool)
        for first, count, _ in ranges:
            keep[first:first + count] = False
        sub = np.ascontiguousarray(idx.reshape(-1, 3)[keep].ravel())
        view = abi.Scene.from_buffer_copy(sc.view)
        view.idxList = C.cast(sub.ctypes.data, C.POINTER(C.c_uint32)); view.n_index = len(sub)
        view.triList = C.cast(vertices.ctypes.data, C.POINTER(abi.TriangleVertex))
        return view, (sub, vertices)

    def timed(call, t):
        t.synchronize()
        t0 = time.perf_counter(); call(); t.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def line(name, xs, unit="ms wall"):
        say(f"   {name:66s}{med(xs):9.3f} {unit} (min {min(xs):.3f}, max {max(xs):.3f})")

    res = {}

    def add(key, value):
        res.setdefault(key, []).append(value)

    with Tracer(0) as new, Tracer(0) as old:
        new.upload_scene_device(sc.view, FLAGS); old.upload_scene_device(sc.view, FLAGS)
        for r in range(a.reps + 1):                                                      # repetition 0 is the warm-up
            keep = r > 0
            for flags, name in ((abi.TREE_SAH, "sah"), (0, "lbvh")):
                ms = timed(lambda: new.rebuild_tree(flags), new)
                if keep:
                    add(("a", name, "wall"), ms); add(("a", name, "dev"), new.lbvh_info()[2])
            ms = timed(lambda: new.set_triangle_visibility([], 0), new)
            if keep:
                add(("b", "nothing hidden (LBVH)", "wall"), ms); add(("b", "nothing hidden (LBVH)", "dev"), new.lbvh_info()[2])
                add(("b", "nothing hidden (LBVH)", "leaf"), new.visibility_ms())
            for name, ranges in subsets.items():
                ms = timed(lambda: new.set_triangle_visibility(ranges, abi.TREE_SAH), new)
                n_leaves = (new.lbvh_info()[0] + 1) // 2
                if keep:
                    add(("b", name, "wall"), ms); add(("b", name, "dev"), new.lbvh_info()[2]); add(("b", name, "leaf"), new.visibility_ms())
                    res[("b", name, "n")] = n_leaves
                if ranges:
                    ms = timed(lambda: new.set_triangle_visibility(everything, abi.TREE_SAH), new)
                    if keep:
                        add(("b", "all shown again after: " + name, "wall"), ms); add(("b", "all shown again after: " + name, "dev"), new.lbvh_info()[2])
                        add(("b", "all shown again after: " + name, "leaf"), new.visibility_ms())

                def route():
                    v = old.download_vertices()
                    view, alive = subset_view(ranges, v)
                    old.upload_scene_device(view, FLAGS)
                    return alive
                ms = timed(route, old)
                if keep:
                    add(("c", name, "wall"), ms); add(("c", name, "dev"), old.lbvh_info()[2])
                old.upload_scene_device(sc.view, FLAGS)                                  # the route's next repetition starts from the whole scene
    say(f"a. trc_rebuild_tree + synchronize, the parent's code, medians of {a.reps}:")
    for name in ("sah", "lbvh"):
        line(f"rebuild_tree({'SAH' if name == 'sah' else '0'})", res[("a", name, "wall")])
        line("   its device time (lbvh_info)", res[("a", name, "dev")], "ms device")
    spread = max(res[("a", "sah", "dev")]) - min(res[("a", "sah", "dev")])
    say(f"   run-to-run spread of the SAH rebuild's device time: {spread:.3f} ms")
    say(f"b. trc_set_triangle_visibility + synchronize, medians of {a.reps}:")
    for key in [k for k in res if k[0] == "b" and k[2] == "wall"]:
        name = key[1]
        n_note = f", {res[('b', name, 'n')]} leaves" if ("b", name, "n") in res else ""
        line(name + n_note, res[key])
        line("   its device time (lbvh_info)", res[("b", name, "dev")], "ms device")
        line("   of it the leaf-list stage (mask, partition, leaf records)", res[("b", name, "leaf")], "ms device")
    base = med(res[("a", "sah", "dev")])
    got, leaf = med(res[("b", "nothing hidden", "dev")]), med(res[("b", "nothing hidden", "leaf")])
    say(f"   nothing hidden (SAH): {got:.3f} ms device against rebuild {base:.3f} + leaf-list stage {leaf:.3f} = {base + leaf:.3f}: "
        f"{got - base - leaf:+.3f} ms, spread of the rebuild {spread:.3f}")
    say(f"c. trc_download_vertices + trc_upload_scene_device of the subset, medians of {a.reps}:")
    for name in subsets:
        line(name, res[("c", name, "wall")])
        line("   the upload's device build time (lbvh_info)", res[("c", name, "dev")], "ms device")
        say(f"      wall ratio route / call {med(res[('c', name, 'wall')]) / med(res[('b', name, 'wall')]):.2f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
