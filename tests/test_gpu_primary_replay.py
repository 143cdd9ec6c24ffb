"""Primary replay (render_block, trc_render_config.hpp): the tracePath production kernels keep the hit of a pixel's camera ray after
the first walk of a launch and answer every later sample's identical camera ray from that memo.  The frame, the RNG texture and
trc_stats.rays must not know: knob no_primary_replay (every camera ray walks) gives the same bits, the oracle too, and
trc_debug_primary_replays counts exactly the camera rays that were not walked.

Kernels: k_render_dense needs a launch list of at least 4 blocks per wavefront slot, i.e. a frame near 1080p (here 1916x1076:
partial blocks on both edges); k_render_pwg<tracePath> runs any mesh scene at >= 8 samples per launch, whatever the frame size."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tracer_amd import abi, host

pytestmark = pytest.mark.gpu

SPP = 8                       # per launch: one kernel launch per trc_render call (no cold head below 16 samples)
STAT_FIELDS = ["paths", "rays", "shaded", "n_descend", "n_return", "n_leaf_sphere", "n_leaf_square", "n_leaf_cube",
               "n_leaf_triangle", "n_hit_triangle", "n_hit_cube"]


def _scenes():
    return {"config2_dense": (lambda: host.HostScene(abi.SCENE_CORNELL_SPHERES), 1916, 1076),
            "teapot_mesh_pwg": (lambda: host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("teapot")), 100, 68)}


def _two_launches(gpu, no_replay, seed=0xFACE):
    """two consecutive launches of SPP samples, the frame counter continuing; replays and rays per launch"""
    gpu.debug_set("no_primary_replay", 1 if no_replay else 0)
    gpu.seed(seed); gpu.clear_accum()
    per_launch = []
    for launch in range(2):
        gpu.reset_stats()
        gpu.render(spp=SPP, frame0=launch * SPP)
        st = gpu.stats()
        assert st.launches == 1
        per_launch.append((st.paths, st.rays, gpu.primary_replays()))
    return gpu.download_accum(), gpu.download_rng(), per_launch


@pytest.mark.parametrize("which", sorted(_scenes()))
def test_replay_changes_no_bit_and_counts_every_camera_ray_it_answers(gpu, which):
    make, W, H = _scenes()[which]
    scene = make()
    gpu.upload_scene(scene.view); gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    try:
        acc_on, rng_on, on = _two_launches(gpu, no_replay=False)
        acc_off, rng_off, off = _two_launches(gpu, no_replay=True)
    finally:
        gpu.debug_set("no_primary_replay", 0)
    print(which, "knob on (paths, rays, replays) per launch:", on, "knob off:", off)
    assert np.array_equal(acc_on.view(np.uint32), acc_off.view(np.uint32))
    assert np.array_equal(rng_on, rng_off)
    for (paths, rays, replays), (paths_off, rays_off, replays_off) in zip(on, off):
        assert paths == paths_off == W * H * SPP and rays == rays_off
        assert replays_off == 0
        # the default camera has aperture 0: every sample after a pixel's first repeats its camera ray.  Short of that only by
        # samples whose origin bits differed (both lens draws exactly 0.5: expected never)
        expected = paths - W * H
        assert replays <= expected and replays >= 0.999 * expected, (replays, expected)


@pytest.mark.parametrize("which", sorted(_scenes()))
def test_a_lens_never_replays_and_the_frame_is_the_oracles(gpu, which):
    make, W, H = _scenes()[which]
    scene = make()
    cam = host.make_camera((278, 278, -800), (278, 278, 278), (0, 1, 0), 0.5, W / H, float(np.deg2rad(45.0)), 10.0)     # the default view through a lens of radius 0.25
    nranks = 64 if W * H > 100000 else 1              # the oracle re-renders 1 tile in 64 of the large frame
    gpu.upload_scene(scene.view); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(31337); gpu.clear_accum(); gpu.reset_stats()
    gpu.render(spp=SPP)
    dev, st, replays = gpu.download_accum(), gpu.stats(), gpu.primary_replays()
    assert st.paths == W * H * SPP and replays == 0
    ref, rst = po.render(scene.view, cam, W, H, host.fill_rng(31337, W, H), spp=SPP, tile_rank=0, tile_nranks=nranks)
    ty, tx = np.mgrid[0:H, 0:W] // abi.TRC_TILE
    mine = ((tx + ty) % nranks) == 0
    assert mine.sum() > 5000 and rst.rays > 0 and (nranks > 1 or st.rays == rst.rays)
    assert np.array_equal(dev[mine].view(np.uint32), ref[mine].view(np.uint32))


@pytest.mark.parametrize("which", sorted(_scenes()))
def test_the_instrumented_launch_walks_every_ray(gpu, which):
    """TRC_FLAG_COLLECT_STATS: the traversal counters are defined on the full walk of every ray"""
    make, _, _ = _scenes()[which]
    scene, W, H = make(), 100, 68
    cam = host.prepare_camera(W, H)
    gpu.upload_scene(scene.view); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(5); gpu.clear_accum(); gpu.reset_stats()
    gpu.render(spp=SPP, collect_stats=True)
    dev, st, replays = gpu.download_accum(), gpu.stats(), gpu.primary_replays()
    ref, rst = po.render(scene.view, cam, W, H, host.fill_rng(5, W, H), spp=SPP)
    assert replays == 0
    for f in STAT_FIELDS:
        assert getattr(st, f) == getattr(rst, f), f
    assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32))
