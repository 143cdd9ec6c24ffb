"""The SVGF stage on the GPU (include/tracer_abi.h "SVGF denoiser", tracer_amd/csrc/trc_denoise.hip): the G-buffer against the
production Scene::hit hook, every plane bit for bit against the CPU restatement (tests/svgf_ref/svgf_ref.cpp), what the
filter buys against a converged render, and that nothing else in the context moves."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_ref"))
import svgf_loader as sl  # noqa: E402

from conftest import camera_rays  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, TracerError  # noqa: E402
from test_svgf_ref import rotated  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sl.build(tmp_path_factory.mktemp("svgf_ref_gpu"))


_SCENES = {}


def scene(config):
    if config not in _SCENES:
        if config in ("2", "5"):
            _SCENES[config] = host.HostScene(abi.SCENE_CORNELL_SPHERES)
        elif config == "3":
            _SCENES[config] = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("coatball"))
        else:
            _SCENES[config] = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("teapot").replicate(8, 80.0))
    return _SCENES[config]


def setup(trc, config, W, H, cam=None):
    trc.upload_scene(scene(config).view)
    trc.set_camera(cam if cam is not None else host.prepare_camera(W, H))
    trc.set_environment((0.0, 0.0, 0.0))
    trc.resize(W, H)
    trc.seed(11)
    if config == "5":
        trc.sppm_init(23)


def advance(trc, config, k):
    """one frame of 1 sample per pixel (SPPM: one photon frame) into the accumulator"""
    if config == "5":
        trc.sppm_frames(1)
    else:
        trc.render(spp=1, frame0=k, integrator=abi.INTEGRATOR_MIS if config == "3" else abi.INTEGRATOR_PATH)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------- G-buffer
@pytest.mark.parametrize("config,step", [("2", 1), ("3", 1), ("4", 3)])
def test_gbuffer_equals_production_scene_hit(gpu, config, step):
    W, H = 160, 96
    setup(gpu, config, W, H)
    gpu.denoise()
    g = gpu.download_gbuffer()
    cam = host.prepare_camera(W, H)
    hits = gpu.trace_rays(camera_rays(cam, W, H, step), production=True)
    g = g[::step, ::step].ravel()
    hit = hits["hit"] != 0
    assert hit.any()
    assert np.array_equal(bits(g["depth"][hit]), bits(hits["t"][hit]))
    assert np.array_equal(bits(g["normal"][hit]), bits(hits["sn"][hit]))
    assert np.array_equal(g["id"][hit], hits["material"][hit])
    assert np.all(np.isposinf(g["depth"][~hit])) and np.all(g["id"][~hit] == abi.GBUFFER_MISS)
    assert np.all(g["albedo"][~hit] == 1.0)
    # albedo = texture_value of the hit material, from the scene's own tables
    view = scene(config).view
    mats = [view.materials[i] for i in range(view.n_material)]
    for m_idx in np.unique(g["id"][hit]):
        sel = g["id"] == m_idx
        m = mats[int(m_idx)]
        alb = np.float32([m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z])
        got = g["albedo"][sel]
        if m.type == abi.MAT_DIFFUSE:
            assert np.all(got == 1.0)                                    # emitters
        elif m.textureInfo.type == 1:                                    # checker: albedo * (0.5 or 1)
            assert np.all(np.all(got == alb, axis=1) | np.all(got == np.float32(0.5) * alb, axis=1))
        else:
            assert np.all(got == alb), (m_idx, got[:3], alb)


# ----------------------------------------------------------------------------------------------------------- bit for bit
def run_sequence(trc, ref, config, W, H, motion, p, n_frames):
    base = host.prepare_camera(W, H)
    setup(trc, config, W, H, base)
    ref.reset()
    for k in range(n_frames):
        deg = {"still": 0.0, "step": 0.5 * k, "jump": 0.0 if k < n_frames // 2 else 12.0}[motion]
        cam = rotated(base, deg)
        trc.set_camera(cam)
        advance(trc, config, k)
        trc.denoise(p)
        accum = trc.download_accum()
        g = trc.download_gbuffer()
        out = trc.download_denoised()
        integ, hist, mom = trc.denoise_state()
        r_integ, r_hist, r_mom, r_out = ref.frame(sl.params(**{f: getattr(p, f) for f, _ in p._fields_}), sl.cam_vectors(cam), g, accum)
        for what, a, b in (("integrated", integ, r_integ), ("history", hist, r_hist), ("moments", mom, r_mom), ("out", out, r_out)):
            bad = bits(a) != bits(b)
            assert not bad.any(), (f"{config} {motion} frame {k}: {what} differs in {int(bad.any(-1).sum())} pixels",
                                   a[bad.any(-1)][:3], b[bad.any(-1)][:3])
    return mom


CASES = [("2", "still", False, 5, (173, 97)), ("2", "step", True, 5, (320, 180)), ("2", "jump", False, 1, (173, 97)),
         ("3", "still", True, 1, (173, 97)), ("3", "step", False, 0, (173, 97)), ("3", "jump", True, 5, (320, 180)),
         ("5", "still", False, 0, (320, 180)), ("5", "step", True, 5, (173, 97)), ("5", "jump", False, 5, (173, 97)),
         ("2", "step", False, 0, (320, 180)), ("2", "still", True, 1, (320, 180))]


@pytest.mark.parametrize("config,motion,demod,iters,size", CASES)
def test_denoised_frame_equals_restatement(gpu_hooks, ref, config, motion, demod, iters, size):
    W, H = size
    p = gpu_hooks.denoise_params(demodulate=demod, iterations=iters)
    mom = run_sequence(gpu_hooks, ref, config, W, H, motion, p, 8)
    if motion == "still":
        # every hit pixel whose normal passes the consistency test with itself (interpolated mesh normals need not be unit) has
        # reprojected onto itself every frame
        g = gpu_hooks.download_gbuffer()
        n = g["normal"]
        self_ok = np.isfinite(g["depth"]) & ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2] >= np.float32(0.9))
        assert self_ok.mean() > 0.3 and np.all(mom[..., 2][self_ok] == 8.0)


def test_full_size_frame_equals_restatement(gpu_hooks, ref):
    p = gpu_hooks.denoise_params(demodulate=True)
    run_sequence(gpu_hooks, ref, "2", 1920, 1080, "step", p, 2)


# ----------------------------------------------------------------------------------------------------------- quality
# K: the ratio measured on an MI355X was 0.091 (raw 1-spp RMSE 0.504, denoised 0.140 after 1 frame, 0.046 after 8); the bound
# leaves room for other seeds.  The ratio is printed so that the bound can be re-checked.
QUALITY_K = 0.15


def test_denoising_lowers_the_error_against_a_converged_render(gpu):
    W, H = 480, 270
    setup(gpu, "2", W, H)
    gpu.seed(1234)
    gpu.render(spp=4096)
    truth = gpu.download_accum()[..., :3].astype(np.float64)
    gpu.seed(5)
    gpu.clear_accum()
    rmse = lambda a: float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - truth) ** 2)))
    errs = []
    for k in range(8):
        gpu.render(spp=1, frame0=k)
        if k == 0:
            raw1 = rmse(gpu.download_accum())
        gpu.denoise()
        errs.append(rmse(gpu.download_denoised()))
    print(f"raw 1 spp RMSE {raw1:.5f}; denoised after 1 frame {errs[0]:.5f}, after 8 {errs[-1]:.5f}; ratio {errs[-1] / raw1:.3f}")
    assert errs[-1] < errs[0]
    assert errs[-1] <= QUALITY_K * raw1


# ----------------------------------------------------------------------------------------------------------- nothing else moves
def test_accumulator_rng_and_next_render_untouched(gpu):
    from oracle import pyoracle as po
    W, H, spp, seed = 64, 48, 4, 42
    setup(gpu, "2", W, H)
    gpu.seed(seed)
    gpu.render(spp=spp)
    acc, rng = gpu.download_accum(), gpu.download_rng()
    gpu.denoise(gpu.denoise_params(demodulate=True))
    gpu.denoise()
    assert np.array_equal(bits(gpu.download_accum()), bits(acc)) and np.array_equal(gpu.download_rng(), rng)
    gpu.seed(seed)
    gpu.clear_accum()
    gpu.denoise()
    gpu.render(spp=spp)
    ref_frame, _ = po.render(scene("2").view, host.prepare_camera(W, H), W, H, host.fill_rng(seed, W, H), spp=spp)
    assert np.array_equal(bits(gpu.download_accum()), bits(ref_frame))
    img, e = gpu.tonemap_denoised()
    assert img.shape == (H, W, 4) and 0 < e <= 1


def test_two_contexts_denoise_independently(ref):
    W, H = 96, 64
    outs = []
    with Tracer(0) as a, Tracer(0) as b:
        for t, s in ((a, 3), (b, 4)):
            setup(t, "2", W, H)
            t.seed(s)
        base = host.prepare_camera(W, H)
        refs = [sl.Ref(ref.L), sl.Ref(ref.L)]
        for k in range(4):
            for t, r in ((a, refs[0]), (b, refs[1])):
                cam = rotated(base, 0.5 * k)
                t.set_camera(cam)
                t.render(spp=1, frame0=k)
                t.denoise()
            for t, r in ((a, refs[0]), (b, refs[1])):
                cam = rotated(base, 0.5 * k)
                _, _, _, r_out = r.frame(sl.params(), sl.cam_vectors(cam), t.download_gbuffer(), t.download_accum())
                assert np.array_equal(bits(t.download_denoised()), bits(r_out))
            outs.append((a.download_denoised(), b.download_denoised()))
    assert not np.array_equal(outs[-1][0], outs[-1][1])


# ----------------------------------------------------------------------------------------------------------- lifecycle
def _history(trc):
    g = trc.download_gbuffer()
    return trc.denoise_state()[2][..., 2][np.isfinite(g["depth"])]


@pytest.mark.parametrize("trigger", ["resize", "upload_scene", "upload_scene_lbvh", "set_environment", "set_environment_map", "denoise_reset"])
def test_every_reset_trigger_drops_the_history(gpu_hooks, trigger):
    W, H = 64, 48
    setup(gpu_hooks, "2", W, H)
    for k in range(3):
        gpu_hooks.render(spp=1, frame0=k)
        gpu_hooks.denoise()
    assert np.all(_history(gpu_hooks) == 3.0)
    if trigger == "resize":
        gpu_hooks.resize(W, H); gpu_hooks.seed(1)
    elif trigger == "upload_scene":
        gpu_hooks.upload_scene(scene("2").view)
    elif trigger == "upload_scene_lbvh":
        gpu_hooks.upload_scene_lbvh(scene("2").leaves_view())
    elif trigger == "set_environment":
        gpu_hooks.set_environment((0.0, 0.0, 0.0))
    elif trigger == "set_environment_map":
        gpu_hooks.set_environment_map(None)
    else:
        gpu_hooks.denoise_reset()
    gpu_hooks.render(spp=1)
    gpu_hooks.denoise()
    assert np.all(_history(gpu_hooks) == 1.0)
    gpu_hooks.render(spp=1, frame0=1)
    gpu_hooks.denoise()
    assert np.all(_history(gpu_hooks) == 2.0)


def test_error_codes():
    with Tracer(0) as t:
        for call in (lambda: t.denoise(), t.download_denoised, t.download_gbuffer, t.tonemap_denoised):
            with pytest.raises(TracerError) as e:
                call()
            assert e.value.status == abi.ERR_NO_FRAME
        t.resize(32, 32)
        with pytest.raises(TracerError) as e:
            t.denoise()
        assert e.value.status == abi.ERR_NO_SCENE
        setup(t, "2", 32, 32)
        for bad in (dict(iterations=6), dict(normal_exponent=100), dict(normal_exponent=0), dict(alpha_color=0.0),
                    dict(alpha_moments=1.5), dict(sigma_z=0.0), dict(sigma_l=-1.0), dict(min_history=0), dict(flags=2)):
            with pytest.raises(TracerError) as e:
                t.denoise(**bad)
            assert e.value.status == abi.ERR_INVALID_ARG, bad
        t.denoise()
        with pytest.raises(TracerError) as e:
            t._check(t._L.trc_denoise(t._h, None), "trc_denoise")
        assert e.value.status == abi.ERR_INVALID_ARG
    # a context in a group: composed frames are not denoised
    from tracer_amd import socket_group as sg

    class Table:
        pass
    tab = Table()
    keep = [sg.REDUCE_FN(lambda *a: 0), sg.ALLREDUCE_FN(lambda *a: 0), sg.ALLGATHER_FN(lambda *a: 0)]
    tab.table = sg.Collectives(None, 1, 0, *keep)
    with Tracer(0) as t:
        setup(t, "2", 32, 32)
        t.set_collectives(tab, 1, 0)
        with pytest.raises(TracerError) as e:
            t.denoise()
        assert e.value.status == abi.ERR_UNSUPPORTED


def test_fast_math_build_agrees_statistically():
    """libtracer_amd_fast.so: approximate division / sqrt / exp and contraction; the denoised frame of the same accumulator
    agrees with the exact build's to 1e-3 relative RMS over the hit pixels (the filter is a weighted mean: no chaos)"""
    W, H = 160, 96
    outs = []
    acc = None
    for fast in (False, True):
        with Tracer(0, fast_math=fast) as t:
            setup(t, "2", W, H)
            if acc is None:
                t.render(spp=1)
                acc = t.download_accum()
            t.upload_accum(acc)
            t.denoise(t.denoise_params(demodulate=True))
            outs.append(t.download_denoised()[..., :3].astype(np.float64))
    rel = np.sqrt(np.mean((outs[0] - outs[1]) ** 2)) / np.sqrt(np.mean(outs[0] ** 2))
    assert rel < 1e-3, rel
