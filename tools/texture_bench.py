#!/usr/bin/env python3
"""What a textured hit costs (trc_upload_textures): each workload with and without image textures on one GPU, the two forms
alternated run by run (as tools/ab_bench.py alternates builds), median and spread per form.

  config 3 (Cornell + coatball.obj, traceMIS, 1920x1080x256spp): the coatball (material 19) an Image of 1024^2 (uv_test.png's size)
           or 4096^2 texels
  config 2 (Cornell + 12 spheres, tracePath, 1920x1080x64spp): every non-emitting wall square an Image of 1024^2 texels

The untextured form is the same scene with no image uploaded: its Image materials resolve to their albedo and the production kernels
run.  The textured one takes the k_render*_tex kernels, with images whose every texel is the material's albedo (up to the last bit
the bilinear blend may round), so both forms trace the same paths: the rays per launch are printed to show it, and the difference is
the lookup and the kernel variant.  (On config 2 the untextured form runs k_render_dense, which has no textured twin.)

  python tools/texture_bench.py [--runs 5] [--configs 3,2]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import workloads  # noqa: E402
from tracer_amd import abi  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402


def texture_scene(wl, config):
    """textureIndex k on the k-th material the case textures; returns their indices"""
    v = wl["scene"].view
    if config == "3":
        mats = [19]
    else:
        mats = sorted({v.squareList[i].material for i in range(v.n_square) if v.materials[v.squareList[i].material].type != abi.MAT_DIFFUSE})
    for k, m in enumerate(mats):
        v.materials[m].textureInfo.type = abi.TEX_IMAGE
        v.materials[m].textureInfo.textureIndex = k
    return mats


def timed(trc, wl, runs_ms, textures):
    trc.upload_textures(textures)
    trc.seed(7); trc.clear_accum(); trc.reset_stats()
    trc.synchronize()
    t0 = time.perf_counter()
    trc.render(spp=wl["spp"], integrator=wl["integrator"])
    trc.synchronize()
    runs_ms.append((time.perf_counter() - t0) * 1e3)
    return trc.stats().rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--configs", default="3,2")
    a = ap.parse_args()
    cases = []
    for c in a.configs.split(","):
        cases += [(c, 1024), (c, 4096)] if c == "3" else [(c, 1024)]
    with Tracer(0) as trc:
        for config, size in cases:
            wl = workloads.make(config)
            mats = texture_scene(wl, config)
            workloads.setup(trc, wl)
            v = wl["scene"].view
            imgs = [np.broadcast_to(np.array([v.materials[m].textureInfo.albedo.x, v.materials[m].textureInfo.albedo.y,
                                              v.materials[m].textureInfo.albedo.z], np.float32), (size, size, 3)).copy() for m in mats]
            plain, tex = [], []
            timed(trc, wl, [], []); timed(trc, wl, [], imgs)              # warm-up of both forms (first-launch planning)
            for _ in range(a.runs):
                rays_plain = timed(trc, wl, plain, [])
                rays_tex = timed(trc, wl, tex, imgs)
            mp, mt = statistics.median(plain), statistics.median(tex)
            print(f"config {config}  {wl['what']}, {wl['spp']} spp, textured materials {mats}, image {size}x{size}")
            print(f"  untextured  median {mp:9.2f} ms   min {min(plain):9.2f}   max {max(plain):9.2f}   runs {' '.join(f'{x:.2f}' for x in plain)}")
            print(f"  textured    median {mt:9.2f} ms   min {min(tex):9.2f}   max {max(tex):9.2f}   runs {' '.join(f'{x:.2f}' for x in tex)}")
            print(f"  textured / untextured (medians): {mt / mp:.4f}   rays per launch {rays_plain} / {rays_tex}")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
