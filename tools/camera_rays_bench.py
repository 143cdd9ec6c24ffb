#!/usr/bin/env python3
"""TRC_FLAG_CAMERA_RAYS measured (profiles/r30/camera_rays.txt), 1920 x 1080 on one MI355X.

  1. the cost of the ray path: a flagged launch of --spp samples (TRC_RAYS_PINHOLE, one set) against the UNFLAGGED launch forced onto the same
     shape (knobs no_dense / no_pwg, strip length 1, primary replay off) and against the production unflagged launch, on config 2 under
     tracePath and traceMIS and on config 4 under tracePath.  One context per side, each with its own settled block costs; the sides take
     turns launch by launch; --warmup launches, then medians of --reps.  Render-kernel time from the launches' event pairs (trc_stats.kernel_ms)
     and wall time between two trc_synchronize.  Every side's frame is compared with the production one's: the same bits.
  2. trc_generate_camera_rays for 1, 16 and 64 sets, and the host generator plus trc_upload_camera_rays of the same; the memory held.
  3. that it anti-aliases: config 2 under traceMIS at --spp samples, unflagged and with as many Halton sets, each against a --truth-spp unflagged
     render at 4 x the resolution in each dimension, box-filtered down (another seed): RMSE of both.
  4. (--steps envlight; profiles/r31/camera_rays_envlight.txt) step 1 for TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT: config 2 under traceMIS with
     an HDR sun-and-sky map as a light, the flag pair against the unflagged TRC_FLAG_ENV_LIGHT launch on the same shape and in production.
  5. (--steps gbuffer) trc_denoise_guide_rays: the G-buffer pass along set 0 of the ray sets against the camera's own, and a whole
     trc_denoise on each side, on config 2 and config 4.  Wall time between two trc_synchronize around a trc_denoise that rebuilds the
     G-buffer (a fresh generation of the same rays on the guided side, a scene upload's invalidation on both) minus one that does not."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workloads  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402

W, H = workloads.W, workloads.H
NAMES = {abi.INTEGRATOR_MIS: "traceMIS", abi.INTEGRATOR_PATH: "tracePath"}
OUT = []


def say(text=""):
    print(text, flush=True)
    OUT.append(text)


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return f"{med(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def timed(t, fn):
    t.synchronize()
    t0 = time.perf_counter()
    fn()
    t.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launch(t, a, integrator, flagged, env_light=False):
    t.seed(a.seed); t.clear_accum(); t.reset_stats()
    wall = timed(t, lambda: t.render(spp=a.spp, integrator=integrator, camera_rays=flagged, env_light=env_light))
    return wall, t.stats().kernel_ms


def sun_sky(w, h, sun=(0.3, 0.7), sun_radius=0.02, sun_power=5000.0):
    """an HDR map: sky by latitude, a disc of sun_power around (u, w) = sun (tools/envlight_bench.py's)"""
    lat = np.pi * ((np.arange(h, dtype=np.float64) + 0.5) / h - 0.5)
    phi = 2 * np.pi * ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5)
    img = np.empty((h, w, 3), np.float32)
    img[:] = 0.05 + np.clip(np.sin(lat), 0, 1)[:, None, None] * np.array([0.4, 0.6, 1.0])
    sp, sl = 2 * np.pi * (sun[0] - 0.5), np.pi * (sun[1] - 0.5)
    cosang = (np.cos(lat)[:, None] * np.cos(phi)[None] * np.cos(sl) * np.cos(sp) + np.sin(lat)[:, None] * np.sin(sl) +
              np.cos(lat)[:, None] * np.sin(phi)[None] * np.cos(sl) * np.sin(sp))
    img[cosang > np.cos(sun_radius)] += sun_power
    return img


def ray_path_cost(a, config, integrator, env_light=False):
    wl = workloads.make(config)
    un = "unflagged" if not env_light else "ENV_LIGHT alone"
    sides = [("flagged, one pinhole set", True, True), (f"{un}, same shape", False, True), (f"{un}, production", False, False)]
    ctxs, res, frames = [], {}, {}
    try:
        for name, flagged, forced in sides:
            t = Tracer(0)
            ctxs.append(t)
            workloads.setup(t, wl)
            if env_light:
                t.set_environment_map(sun_sky(1024, 512))
            if forced:
                for knob in ("no_dense", "no_pwg", "no_primary_replay"):
                    t.debug_set(knob, 1)
                t.debug_set("strip_len", 1)
            if flagged:
                t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
        say(f"--- {wl['what'].split(',')[0]}, {NAMES[integrator]}{' + TRC_FLAG_ENV_LIGHT (1024 x 512 sun-and-sky map)' if env_light else ''}, {W}x{H}, {a.spp} spp per launch; {a.warmup} warm-up launches, medians of {a.reps}")
        for r in range(a.warmup + a.reps):
            order = list(zip(sides, ctxs))
            for (name, flagged, _), t in (order if r % 2 == 0 else order[::-1]):
                wall, kernel = launch(t, a, integrator, flagged, env_light)
                if r >= a.warmup:
                    e = res.setdefault(name, dict(wall=[], kernel=[]))
                    e["wall"].append(wall); e["kernel"].append(kernel)
        for (name, _, _), t in zip(sides, ctxs):
            frames[name] = t.download_accum().view(np.uint32)
        base = med(res[sides[1][0]]["kernel"])
        for name, _, _ in sides:
            e = res[name]
            same = np.array_equal(frames[name], frames[sides[2][0]])
            say(f"   {name:26s} render kernel {spread(e['kernel'])}  wall {spread(e['wall'])}  x{med(e['kernel']) / base:5.3f} of the same shape; "
                f"frame {'==' if same else '!='} production's")
    finally:
        for t in ctxs:
            t.close()


def generator(a):
    say(f"--- camera-ray sets at {W}x{H}: {W * H * 32 / 1e6:.1f} MB per set")
    cam = host.prepare_camera(W, H)
    with Tracer(0) as t:
        workloads.setup(t, workloads.make("2"))
        for n_sets in (1, 16, 64):
            off = host.halton_offsets(n_sets)
            dev = [timed(t, lambda: t.generate_camera_rays(abi.RAYS_PINHOLE, n_sets, off)) for _ in range(a.gen_reps + 1)][1:]
            gen, up = [], []
            for _ in range(a.gen_reps):
                t0 = time.perf_counter()
                rays = host.generate_camera_rays(cam, W, H, abi.RAYS_PINHOLE, n_sets, off)
                gen.append((time.perf_counter() - t0) * 1e3)
                up.append(timed(t, lambda: t.upload_camera_rays(rays)))
            say(f"   {n_sets:3d} sets, {n_sets * W * H * 32 / 1e6:7.1f} MB held: trc_generate_camera_rays {spread(dev)}   "
                f"({n_sets * W * H * 32 / (med(dev) * 1e-3) / 1e9:6.1f} GB/s written)")
            say(f"            trc_host_generate_camera_rays {spread(gen)}  + trc_upload_camera_rays {spread(up)}")
            del rays


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def anti_aliasing(a):
    wl = workloads.make("2")
    K = 4
    say(f"--- config 2, traceMIS, {W}x{H}, {a.spp} spp: RMSE against {a.truth_spp} spp unflagged at {K * W}x{K * H}, box-filtered {K}x{K} (another seed)")
    with Tracer(0) as t:
        t.upload_scene(wl["scene"].view); t.set_camera(host.prepare_camera(K * W, K * H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(K * W, K * H)
        t.seed(a.seed + 1000); t.clear_accum()
        done = 0
        while done < a.truth_spp:                 # launches of 256 samples: a long launch is one long silence
            n = min(256, a.truth_spp - done)
            t.render(spp=n, integrator=abi.INTEGRATOR_MIS, frame0=done); t.synchronize()
            done += n
        truth = t.download_accum()[..., :3].astype(np.float64).reshape(H, K, W, K, 3).mean(axis=(1, 3))
        t.set_camera(host.prepare_camera(W, H)); t.resize(W, H)
        t.seed(a.seed); t.clear_accum()
        t.render(spp=a.spp, integrator=abi.INTEGRATOR_MIS)
        plain = t.download_accum()
        t.generate_camera_rays(abi.RAYS_PINHOLE, a.spp, host.halton_offsets(a.spp))
        t.seed(a.seed); t.clear_accum()
        t.render(spp=a.spp, integrator=abi.INTEGRATOR_MIS, camera_rays=True)
        aa = t.download_accum()
    say(f"   unflagged (every sample through the pixel's corner)  RMSE {rmse(plain, truth):.5f}")
    say(f"   flagged, {a.spp} Halton sets                              RMSE {rmse(aa, truth):.5f}")


def gbuffer_cost(a, config):
    """trc_denoise with a G-buffer rebuild against trc_denoise without one, guided (set 0 of one pinhole set) and unguided"""
    wl = workloads.make(config)
    say(f"--- {wl['what'].split(',')[0]}, {W}x{H}: trc_denoise (5 a-trous iterations, demodulation), wall between two trc_synchronize; medians of {a.reps}")
    for guided in (False, True):
        with Tracer(0) as t:
            workloads.setup(t, wl)
            t.seed(a.seed); t.clear_accum()
            t.render(spp=8, integrator=abi.INTEGRATOR_PATH)
            p = t.denoise_params(demodulate=True)
            if guided:
                t.denoise_guide_rays(True)
                t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
            t.denoise(p); t.synchronize()
            keep, rebuild = [], []
            for r in range(a.warmup + a.reps):
                k = timed(t, lambda: t.denoise(p))                      # the G-buffer stands
                t.denoise_guide_rays(not guided); t.denoise_guide_rays(guided)      # the switch there and back: the G-buffer is stale, on either side
                b = timed(t, lambda: t.denoise(p))
                if r >= a.warmup:
                    keep.append(k); rebuild.append(b)
            say(f"   {'guided by set 0' if guided else 'the camera ray '}  trc_denoise, G-buffer kept {spread(keep)}  rebuilt {spread(rebuild)}  "
                f"k_gbuffer ~ {med(rebuild) - med(keep):6.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gen-reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--steps", default="cost,generator,aa")
    ap.add_argument("--out", default=None, help="the report goes here too")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if "cost" in steps:
        say("1. the cost of the ray path")
        for config, integrator in (("2", abi.INTEGRATOR_PATH), ("2", abi.INTEGRATOR_MIS), ("4", abi.INTEGRATOR_PATH)):
            ray_path_cost(a, config, integrator)
    if "generator" in steps:
        say("2. making the ray sets")
        generator(a)
    if "aa" in steps:
        say("3. that it anti-aliases")
        anti_aliasing(a)
    if "envlight" in steps:
        say("4. the cost of the ray path under TRC_FLAG_ENV_LIGHT")
        ray_path_cost(a, "2", abi.INTEGRATOR_MIS, env_light=True)
    if "gbuffer" in steps:
        say("5. the G-buffer along the rays")
        for config in ("2", "4"):
            gbuffer_cost(a, config)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
