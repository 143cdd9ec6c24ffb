"""How the render kernels sit on a CU (trc_render_pass.hip: resident_workgroups; tracer_amd/csrc/trc_lds_fit.hpp): the launch plans count
the workgroups the RUNTIME says a CU holds of the kernel that runs, with its dynamic LDS, instead of a hand formula -- and the shape
k_render_dense ships in is one the CU really holds at the waves per SIMD it is compiled for.  Pixels know nothing of any of it: the
packed memo word of the 7-row primary replay is held to the frames of knob no_primary_replay, the mesh kernels' refitted LDS plans
to the oracle.

k_render_dense needs a launch list of at least TRC_DENSE_MIN_BLOCKS_PER_SLOT blocks per wavefront slot (trc_debug_last_kernel says
whether it ran): a 1920x1080 frame; 8 samples are the fewest a launch that is no strip takes, about 2 ms."""
import ctypes as C

import numpy as np
import pytest

import light_oracle_cases as lc
from oracle import pyoracle as po
from tracer_amd import abi, host

pytestmark = pytest.mark.gpu

W, H, SPP = 1920, 1080, 8


def _checker_cube_view(scene):
    """the scene with every cube's material made a checker texture: its colour reads rec.uv, which 7 or 8 memo rows do not keep"""
    v = abi.Scene.from_buffer_copy(scene.view)
    mats = (abi.Material * v.n_material)(*[v.materials[i] for i in range(v.n_material)])
    assert v.n_cube > 0
    for i in range(v.n_cube):
        mats[v.cubeList[i].material].textureInfo.type = abi.TEX_CHECKER
    v.materials = C.cast(mats, C.POINTER(abi.Material))
    return v, mats                                     # (the caller keeps `mats` alive)


def _two_launches(t, no_replay):
    """8 + 8 samples, the second launch's frame0 following on: (accumulator bits, RNG texture, per launch (paths, rays, replays))"""
    t.debug_set("no_primary_replay", 1 if no_replay else 0)
    t.seed(0xD15C); t.clear_accum()
    per_launch = []
    for launch in range(2):
        t.reset_stats()
        t.render(spp=SPP, frame0=launch * SPP)
        st = t.stats()
        assert st.launches == 1
        per_launch.append((st.paths, st.rays, t.primary_replays()))
    return t.download_accum().view(np.uint32), t.download_rng(), per_launch


def _on_and_off(t, view):
    t.upload_scene(view); t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    try:
        on = _two_launches(t, no_replay=False)
        kernel, fit, shape = t.last_kernel(), t.last_residency(), t.launch_shape()
        off = _two_launches(t, no_replay=True)
    finally:
        t.debug_set("no_primary_replay", 0)
    return dict(on=on, off=off, kernel=kernel, fit=fit, shape=shape)


@pytest.fixture(scope="module")
def plain(gpu_hooks):
    scene = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    return _on_and_off(gpu_hooks, scene.view)


@pytest.fixture(scope="module")
def checker(gpu_hooks):
    scene = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    view, mats = _checker_cube_view(scene)
    res = _on_and_off(gpu_hooks, view)
    # what every pixel's camera ray meets, from the oracle: the replay count is predicted from it (tests/test_gpu_primary_replay.py)
    res["hits"] = lc.primary_hits(lc.SceneSet(scene, None, view=view), host.prepare_camera(W, H), W, H)
    return res


def test_wave_slots_are_what_the_runtime_says_the_cu_holds(plain):
    kernel, fit, shape = plain["kernel"], plain["fit"], plain["shape"]
    print("kernel", kernel, "residency", fit, "wave_slots", shape["wave_slots"])
    assert kernel["shape"] == "dense" and kernel["lds_resident"]              # the criterion admitted this frame
    assert fit["block"] == 64 and fit["per_cu"] > 0 and fit["per_cu"] == fit["planned_with"]
    assert shape["wave_slots"] == fit["cu_count"] * fit["per_cu"]
    # the shape the kernel ships in: the CU holds what the kernel is compiled for -- the plan and the machine agree
    assert fit["planned_per_cu"] == 4 * fit["waves"]
    assert shape["wave_slots"] == fit["cu_count"] * 4 * fit["waves"]
    # ... and would still if LDS is granted in blocks of 1280 bytes, which the runtime's query does not count
    assert fit["per_cu_block1280"] >= 4 * fit["waves"]


@pytest.mark.parametrize("which", ["plain", "checker"])
def test_replay_on_and_off_give_the_same_bits(request, which):
    """the memo's packed word (material | side | tag, or the replay count of a column that lost its record) changes no bit of the
    frame, of the RNG texture or of the ray count; with a checker texture on the cubes their pixels walk where the memo has no rows
    for uv (7, 8) and replay where it has (10) -- the same bits either way"""
    res = request.getfixturevalue(which)
    (acc_on, rng_on, on), (acc_off, rng_off, off) = res["on"], res["off"]
    print(which, "replay on (paths, rays, replays) per launch:", on, "off:", off, "kernel", res["kernel"])
    assert res["kernel"]["shape"] == "dense"
    assert np.array_equal(acc_on, acc_off) and np.array_equal(rng_on, rng_off)
    for (paths, rays, replays), (paths_off, rays_off, replays_off) in zip(on, off):
        assert paths == paths_off == W * H * SPP and rays == rays_off and replays_off == 0
        expected = paths - W * H                      # aperture 0: every sample after a pixel's first repeats its camera ray
        if which == "plain":
            assert replays == expected
        elif res["fit"]["dense_memo_rows"] >= 10:
            assert replays == expected                # uv has rows: the cubes' pixels replay too
        else:                                         # checker cubes are in view, and exactly their pixels walk every sample
            assert replays == (SPP - 1) * int(lc.kept_pixels(res["hits"], res["fit"]["dense_memo_rows"]).sum())
            assert 0 < replays < expected


@pytest.fixture(scope="module")
def teapot():
    scene, Wm, Hm, seed = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("teapot")), 256, 256, 77
    cam = host.prepare_camera(Wm, Hm)
    ref, ref_st = po.render(scene.view, cam, Wm, Hm, host.fill_rng(seed, Wm, Hm), spp=SPP)
    return scene, cam, Wm, Hm, seed, ref.view(np.uint32), ref_st


@pytest.mark.parametrize("shape", ["pwg", "one"])
def test_the_mesh_kernels_hold_what_their_plan_is_for(gpu_hooks, teapot, shape):
    """k_render_pwg (the default on a tree read from memory) and k_render (knob no_pwg): after the plan's check against the runtime the
    CU holds at least the workgroups the plan is for, and the frame is the oracle's"""
    t = gpu_hooks
    scene, cam, Wm, Hm, seed, ref, ref_st = teapot
    t.upload_scene(scene.view); t.set_camera(cam); t.set_environment((0.0, 0.0, 0.0)); t.resize(Wm, Hm)
    t.debug_set("no_pwg", 1 if shape == "one" else 0)
    try:
        t.seed(seed); t.clear_accum(); t.reset_stats()
        t.render(spp=SPP)
        dev, st, kernel, fit = t.download_accum().view(np.uint32), t.stats(), t.last_kernel(), t.last_residency()
    finally:
        t.debug_set("no_pwg", 0)
    print(shape, "kernel", kernel, "residency", fit)
    assert kernel["shape"] == shape and not kernel["lds_resident"]
    assert fit["per_cu"] >= fit["planned_per_cu"] > 0 and fit["per_cu"] == fit["planned_with"]
    assert st.rays == ref_st.rays and np.array_equal(dev, ref)
