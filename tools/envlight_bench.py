#!/usr/bin/env python3
"""What TRC_FLAG_ENV_LIGHT costs and buys, on one GPU:

  1. table build: the GPU time of trc_envlight.hip's three kernels (trc_debug_env_tables' build_ms) for synthetic sun + sky maps of
     1024x512, 4096x2048 and 8192x4096, three builds each
  2. ms per launch with the flag off and on, config 3's scene (Cornell + coatball.obj, traceMIS, 1920x1080x256spp) under a 4096x2048
     sun + sky map, the two forms alternated run by run, median and spread
  3. equal-time RMSE against a high-spp reference, at 480x270 on the same scene and map: each form gets the samples that fit the
     time the flag-off form takes for 64 spp (time per sample measured at that size); reference = 4096 flag-off samples, another seed

  python tools/envlight_bench.py [--runs 5]     (needs libtracer_amd_hooks.so for the build times)
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import workloads  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402


def sun_sky(W, H, sun=(0.3, 0.7), sun_radius=0.02, sun_power=5000.0):
    """float32 sun + sky map built row by row (cheap at 8192x4096): sky by latitude, a disc of sun_power around (u, w) = sun"""
    w = (np.arange(H, dtype=np.float32) + 0.5) / H
    lat = np.pi * (w - 0.5)
    up = np.clip(np.sin(lat), 0, 1)
    img = np.empty((H, W, 3), np.float32)
    img[:] = (0.05 + up[:, None, None] * np.array([0.4, 0.6, 1.0], np.float32))
    sp, sl = 2 * np.pi * (sun[0] - 0.5), np.pi * (sun[1] - 0.5)
    s = np.array([np.cos(sl) * np.cos(sp), np.sin(sl), np.cos(sl) * np.sin(sp)])
    j0, j1 = int((sun[1] - 2 * sun_radius / np.pi) * H), int((sun[1] + 2 * sun_radius / np.pi) * H) + 1
    for j in range(max(j0, 0), min(j1, H)):
        la = lat[j]
        phi = 2 * np.pi * ((np.arange(W) + 0.5) / W - 0.5)
        cosang = np.cos(la) * np.cos(phi) * s[0] + np.sin(la) * s[1] + np.cos(la) * np.sin(phi) * s[2]
        img[j, cosang > np.cos(sun_radius)] += sun_power
    return img


def build_times(runs=3):
    print("1. table build (GPU time of k_env_weights + k_env_rows + k_env_marginal)")
    with Tracer(0, hooks=True) as t:
        for W, H in ((1024, 512), (4096, 2048), (8192, 4096)):
            m = sun_sky(W, H)
            ms = []
            for _ in range(runs):
                t.set_environment_map(m)                      # a new map: the tables are dropped and rebuilt below
                total, b = C.c_double(), C.c_float()
                t._check(t._L.trc_debug_env_tables(t._h, None, None, None, C.byref(total), C.byref(b)), "trc_debug_env_tables")
                ms.append(b.value)
            t.set_environment_map(None)
            print(f"  {W}x{H}: median {statistics.median(ms):8.2f} ms   runs {' '.join(f'{x:.2f}' for x in ms)}")
            sys.stdout.flush()


def launch_times(runs):
    wl = workloads.make("3")
    print(f"2. ms per launch, {wl['what']}, {workloads.W}x{workloads.H}x{wl['spp']} spp, 4096x2048 sun + sky map")
    with Tracer(0) as t:
        workloads.setup(t, wl)
        t.set_environment_map(sun_sky(4096, 2048))

        def timed(flag, out):
            t.seed(7); t.clear_accum(); t.reset_stats(); t.synchronize()
            t0 = time.perf_counter()
            t.render(spp=wl["spp"], integrator=wl["integrator"], env_light=flag)
            t.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
            return t.stats().rays
        timed(False, []); timed(True, [])                     # warm-up of both forms (first-launch planning, the table build)
        off, on = [], []
        for _ in range(runs):
            r_off = timed(False, off)
            r_on = timed(True, on)
        t.set_environment_map(None)
    mo, mn = statistics.median(off), statistics.median(on)
    print(f"  flag off  median {mo:9.2f} ms   min {min(off):9.2f}   max {max(off):9.2f}   rays {r_off}")
    print(f"  flag on   median {mn:9.2f} ms   min {min(on):9.2f}   max {max(on):9.2f}   rays {r_on}")
    print(f"  on / off (medians): {mn / mo:.4f}")
    sys.stdout.flush()


def equal_time_rmse():
    wl = workloads.make("3")
    W, H = 480, 270
    print(f"3. equal-time RMSE, {wl['what']}, {W}x{H}, 4096x2048 sun + sky map")
    with Tracer(0) as t:
        t.upload_scene(wl["scene"].view)
        t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
        t.set_environment_map(sun_sky(4096, 2048))

        def frame(flag, spp, seed):
            t.seed(seed); t.clear_accum(); t.synchronize()
            t0 = time.perf_counter()
            t.render(spp=spp, integrator=abi.INTEGRATOR_MIS, env_light=flag)
            t.synchronize()
            return t.download_accum()[..., :3].astype(np.float64), (time.perf_counter() - t0) * 1e3
        ref, ref_ms = frame(False, 4096, 1234)
        frame(True, 64, 5)                                    # table build + planning out of the timed runs
        per = {f: min(frame(f, 256, 5)[1] for _ in range(2)) / 256 for f in (False, True)}
        budget = 64 * per[False]
        for f in (False, True):
            spp = max(1, int(round(budget / per[f])))
            img, ms = frame(f, spp, 99)
            rmse = float(np.sqrt(((img - ref) ** 2).mean()))
            print(f"  flag {'on ' if f else 'off'}: {per[f]:.4f} ms per sample, {spp:4d} spp in {ms:7.2f} ms, RMSE {rmse:.5f}")
        print(f"  reference: 4096 spp flag off in {ref_ms:.1f} ms, mean {ref.mean():.5f}")
        t.set_environment_map(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    build_times()
    launch_times(a.runs)
    equal_time_rmse()


if __name__ == "__main__":
    main()
