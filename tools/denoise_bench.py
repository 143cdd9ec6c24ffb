"""SVGF stage at 1920x1080 (trc_denoise): ms per call for config 2 (1 spp per frame, camera stepping 0.5 degrees per frame, so every
call rebuilds the G-buffer and reprojects) and config 5 (SPPM frames, still camera: G-buffer cached, identity reprojection), and
the compulsory bytes per pixel of each kernel.  One JSON line.  Per-kernel times: run under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/denoise_bench.py
(k_gbuffer, k_svgf_temporal, k_svgf_atrous, k_svgf_finish)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402

# compulsory DRAM-side bytes per pixel (float4 planes; the G-buffer texel is 32 B, a tap reads its first 16)
BYTES_PER_PIXEL = {
    "k_gbuffer": 32,                        # write (the walk's scene reads are not counted)
    "k_svgf_temporal_still": 16 + 32 + 16 + 32 + 32,     # accum, G-buffer, previous texel's id half + depth half, history colour + moments, 2 writes
    "k_svgf_temporal_moving": 16 + 32 + 4 * (32 + 32) + 32,
    "k_svgf_atrous": 16 + 16 + 16,          # (colour, variance) + depth/normal in, one plane out (the last one: + albedo + accum alpha)
}


def turned(cam, degrees):
    a = np.radians(degrees)
    v = np.array([cam.v.x, cam.v.y, cam.v.z], np.float64)
    v /= np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    out = copy.deepcopy(cam)
    eye = np.array([cam.lookFrom.x, cam.lookFrom.y, cam.lookFrom.z])
    for name, point in (("lookAt", True), ("u", False), ("v", False), ("w", False), ("vertical", False), ("horizontal", False), ("cornerLowLeft", True)):
        f = getattr(cam, name)
        x = np.array([f.x, f.y, f.z])
        y = R @ (x - eye) + eye if point else R @ x
        g = getattr(out, name)
        g.x, g.y, g.z = (float(t) for t in y)
    return out


def timed(trc, fn):
    trc.synchronize()
    t0 = time.perf_counter()
    fn()
    trc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    W, H = a.width, a.height
    out = {"width": W, "height": H, "frames": a.frames, "bytes_per_pixel": BYTES_PER_PIXEL}
    with Tracer(0) as trc:
        scene = host.HostScene(abi.SCENE_CORNELL_SPHERES)          # owns the arrays the view points at
        trc.upload_scene(scene.view)
        base = host.prepare_camera(W, H)
        trc.set_camera(base)
        trc.set_environment((0.0, 0.0, 0.0))
        trc.resize(W, H)
        trc.seed(7)
        render, denoise = [], []
        for k in range(a.frames):
            trc.set_camera(turned(base, 0.5 * k))
            render.append(timed(trc, lambda: trc.render(spp=1, frame0=0)))
            denoise.append(timed(trc, lambda: trc.denoise(trc.denoise_params(demodulate=True))))
        out["config2_moving"] = {"render_ms": float(np.median(render[2:])), "denoise_ms": float(np.median(denoise[2:]))}
        trc.set_camera(base)
        trc.seed(7)
        trc.sppm_init(9)
        sppm, denoise = [], []
        for k in range(a.frames):
            sppm.append(timed(trc, lambda: trc.sppm_frames(1)))
            denoise.append(timed(trc, lambda: trc.denoise()))
        out["config5_still"] = {"sppm_frame_ms": float(np.median(sppm[2:])), "denoise_ms": float(np.median(denoise[2:]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
