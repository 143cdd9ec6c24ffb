"""Primary replay (render_block, trc_render_config.hpp): the tracePath production kernels keep the hit of a pixel's camera ray after
the first walk of a launch and answer every later sample's identical camera ray from that memo.  The frame, the RNG texture and
trc_stats.rays must not know: knob no_primary_replay (every camera ray walks) gives the same bits, the oracle too, and
trc_debug_primary_replays counts exactly the camera rays that were not walked.

Kernels: k_render_dense needs a launch list of at least 4 blocks per wavefront slot, i.e. a frame near 1080p (here 1916x1076:
partial blocks on both edges); k_render_pwg<tracePath> runs any mesh scene at >= 8 samples per launch, whatever the frame size."""
import hashlib

import numpy as np
import pytest

import light_oracle_cases as lc
from oracle import pyoracle as po
from tracer_amd import abi, host
from tracer_amd.device import TracerError

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


# ------------------------------------------------------------------------------------------------------------- the replay matrix
# What the tests above leave open (they render material 19 under a black environment): the per-triangle-material twins, whose memo
# keeps a material that differs from triangle to triangle and whose emitter triangles take the `ends` branch; an escaping camera ray
# that memoises a radiance which is not black (a constant colour, and the map tracePath looks up on a miss); uv through the 10-row
# memo; the two scheduling knobs with values, on kernels that have a memo; blocks of few lanes; tile shares, stacked views, short
# paths, an odd sample count, a second launch onto the first's accumulator, a camera that moves, the cold head and the split parts.
# Every case is tracePath under the PCG sampler and compares replay on, knob no_primary_replay and the oracle bit for bit, names
# its kernel, and holds trc_debug_primary_replays to (spp - 1) x the pixels whose primary hit the memo keeps -- predicted from the
# oracle's trace of every camera ray (light_oracle_cases.primary_hits), never from the GPU.
#
# Scenes (light_oracle_cases.replay_scene, camera replay_camera; tests/test_replay_scenes.py holds the camera to its conditions):
# 61 x 45 on the 1104-triangle ball -- persistent workgroups, 10 memo rows in global memory, every pixel replays; 1916 x 1076 on the
# 12-triangle ball -- k_render_dense, 7 packed rows in LDS, the uv readers walk; the oracle renders one tile in 64 of that frame.
# (The 48-triangle ball of the other LDS-resident tests is refused the dense kernel: its workgroup needs 9408 bytes of LDS, and a CU
# holds the 24 the kernel is compiled for only up to 6826; the 12-triangle one needs 6592.)
# No replay count of the matrix had to be left inexact: with aperture 0 every sample's origin has the eye's bits, so a pixel either
# keeps its record for the whole launch or (a uv reader, under 10 rows) never has one.
RW, RH, RSEED = lc.W, lc.H, 0xBEEF
DW, DH, DENSE_NRANKS = 1916, 1076, 64
PWG_MEMO_ROWS = 10                  # TRC_REPLAY_PWG_PATH (trc_render_config.hpp); the dense kernel's rows come from trc_debug_last_residency
PWG_SCENES = {"trimat": ("trimat", "plain"), "tex": ("plain", "tex"), "trimat+tex": ("trimat", "tex")}       # -> (family, variant)
DENSE_SCENES = ["dense-trimat", "dense-trimat-checker"]
ENVS = ["rgb", "spiky"]
FAULTED = []                        # the run whose launch left an error behind: nothing more of the matrix runs on the GPU after it
_RUNS, _REFS, _HITS, _ON_DEVICE = {}, {}, {}, {}


class Spec:
    """one case of the matrix: the scene, the environment (`rgb`: the constant colour; `spiky`: that map over it), the frame, the
    launches as (spp, frame0, camera 0 | 1), and what trc_render is told besides"""

    def __init__(self, scene, env="rgb", W=RW, H=RH, launches=((SPP, 0, 0),), max_depth=8, small_blocks=None, tile=(0, 1), view_height=0):
        self.scene, self.env, self.W, self.H, self.launches = scene, env, W, H, tuple(launches)
        self.max_depth, self.small_blocks, self.tile, self.view_height = max_depth, small_blocks, tuple(tile), view_height
        self.dense = scene.startswith("dense")
        self.oracle_tile = (0, DENSE_NRANKS) if self.dense else self.tile          # the oracle renders one tile in 64 of the large frame

    def key(self):
        return (self.scene, self.env, self.W, self.H, self.launches, self.max_depth, self.small_blocks, self.tile, self.view_height)

    def camera(self, which):
        return lc.replay_camera(self.W, self.H, which)

    def mask(self, tile):
        ty, tx = np.mgrid[0:self.H, 0:self.W] // abi.TRC_TILE
        return ((tx + ty) % tile[1]) == tile[0]

    def hits(self, which):
        key = (self.scene, self.W, self.H, self.view_height, which)
        if key not in _HITS:
            _HITS[key] = lc.primary_hits(lc.replay_scene(self.scene), self.camera(which), self.W, self.H, self.view_height)
        return _HITS[key]


@pytest.fixture(scope="module")
def rgpu(gpu_hooks):
    yield gpu_hooks
    if not FAULTED:
        gpu_hooks.upload_triangle_materials(None); gpu_hooks.upload_textures([]); gpu_hooks.set_environment_map(None)
        gpu_hooks.set_environment((0.0, 0.0, 0.0))


def _ensure_on_device(t, spec):
    """one upload per scene (and per map, and per frame size) for the cases that follow each other"""
    if _ON_DEVICE.get("scene") != spec.scene:
        s = lc.replay_scene(spec.scene)
        t.upload_scene(s.view); t.upload_triangle_materials(s.tri); t.upload_textures(s.images)
        _ON_DEVICE.update(scene=spec.scene, env=None, size=None)
    if _ON_DEVICE.get("env") != spec.env:
        t.set_environment(lc.ENV_RGB)
        t.set_environment_map(lc.env_map("spiky") if spec.env == "spiky" else None)
        _ON_DEVICE["env"] = spec.env
    if _ON_DEVICE.get("size") != (spec.W, spec.H):
        t.resize(spec.W, spec.H)
        _ON_DEVICE["size"] = (spec.W, spec.H)


def _keep(spec, acc, rng):
    """what a run keeps of its frame: all of a small one; of the large one the pixels the oracle renders, and a digest of the rest"""
    if not spec.dense:
        return acc, rng, None
    cmp = spec.mask(spec.oracle_tile)
    return acc[cmp], rng[cmp], hashlib.sha256(acc.tobytes() + rng.tobytes()).hexdigest()


def _run(t, spec, no_replay=False, min_lanes=0, chain=0):
    """the case on the GPU -> accumulator bits, RNG texture, digest, per launch (paths, rays, shaded, replays, kernel choice, residency);
    min_lanes / chain: knobs replay_min_lanes / replay_chain (0: the library's defaults)"""
    key = (spec.key(), no_replay, min_lanes, chain)
    if key in _RUNS:
        return _RUNS[key]
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    try:
        _ensure_on_device(t, spec)
        t.debug_set("no_primary_replay", 1 if no_replay else 0)
        t.debug_set("replay_min_lanes", min_lanes); t.debug_set("replay_chain", chain)
        t.seed(RSEED); t.clear_accum()
        per_launch = []
        for spp, frame0, which in spec.launches:
            t.set_camera(spec.camera(which)); t.reset_stats()
            t.render(spp=spp, frame0=frame0, max_depth=spec.max_depth, integrator=abi.INTEGRATOR_PATH, small_blocks=spec.small_blocks,
                     tile_rank=spec.tile[0], tile_nranks=spec.tile[1], view_height=spec.view_height)
            st = t.stats()
            assert st.launches == 1
            per_launch.append((st.paths, st.rays, st.shaded, t.primary_replays(), t.last_kernel(), t.last_residency()))
        acc, rng = t.download_accum(), t.download_rng()
        assert np.isfinite(acc).all()
        out = _keep(spec, acc.view(np.uint32), rng) + (per_launch,)
        # (not in a `finally`: after a TracerError, a device fault included, nothing more is asked of this context)
        t.debug_set("no_primary_replay", 0); t.debug_set("replay_min_lanes", 0); t.debug_set("replay_chain", 0)
    except TracerError:
        FAULTED.append(repr(key))
        raise
    _RUNS[key] = out
    return out


def _oracle(spec):
    """the case in the oracle, on its share of the tiles -> accumulator bits, RNG texture, per launch (paths, rays, shaded)"""
    if spec.key() not in _REFS:
        s = lc.replay_scene(spec.scene)
        po.set_environment_map(lc.env_map("spiky") if spec.env == "spiky" else None)
        try:
            rng, acc, per_launch = host.fill_rng(RSEED, spec.W, spec.H), None, []
            for spp, frame0, which in spec.launches:
                acc, st = po.render(s.view, spec.camera(which), spec.W, spec.H, rng, accum=acc, spp=spp, frame0=frame0, max_depth=spec.max_depth,
                                    env=lc.ENV_RGB, triangle_materials=s.tri, textures=s.images, tile_rank=spec.oracle_tile[0],
                                    tile_nranks=spec.oracle_tile[1], view_height=spec.view_height)
                per_launch.append((st.paths, st.rays, st.shaded))
        finally:
            po.set_environment_map(None)
        _REFS[spec.key()] = _keep(spec, acc.view(np.uint32), rng)[:2] + (per_launch,)
    return _REFS[spec.key()]


def _expected_replays(spec, launch, kernel, fit):
    """(spp - 1) x the pixels of this launch whose primary hit the memo keeps, from the oracle's trace of every camera ray"""
    spp, _, which = spec.launches[launch]
    rows = fit["dense_memo_rows"] if kernel["shape"] == "dense" else PWG_MEMO_ROWS
    assert rows in (7, 8, 10)
    return (spp - 1) * int((lc.kept_pixels(spec.hits(which), rows) & spec.mask(spec.tile)).sum())


def _same_run(a, b):
    """the same frame, RNG texture, paths / rays / shaded and replays per launch"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert [l[:4] for l in a[3]] == [l[:4] for l in b[3]]


def _verify(t, spec, exact=True, **knobs):
    """replay on (under the knobs), knob no_primary_replay and the oracle: the same bits; the kernel is the one the case is for;
    replays is the predicted count (exact=False, the cold head: bounded by it)"""
    on, off, ref = _run(t, spec, **knobs), _run(t, spec, no_replay=True), _oracle(spec)
    family, variant = ("trimat", "plain") if spec.dense else PWG_SCENES[spec.scene]
    own = spec.mask(spec.tile)
    assert len(on[3]) == len(off[3]) == len(ref[2]) == len(spec.launches)
    for i, ((paths, rays, shaded, replays, kernel, fit), l_off, l_ref) in enumerate(zip(on[3], off[3], ref[2])):
        want = _expected_replays(spec, i, kernel, fit)
        print(f"{spec.key()} {knobs} launch {i}: kernel {kernel['shape']} {kernel['variant']} trimat {kernel['triangle_materials']}; paths {paths} rays {rays} "
              f"shaded {shaded}; replays {replays}, predicted {want}; without replay {l_off[:4]}; oracle {l_ref}")
        assert kernel["shape"] == ("dense" if spec.dense else "pwg") and kernel["variant"] == variant, kernel
        assert kernel["triangle_materials"] == (family == "trimat") and kernel["lds_resident"] == spec.dense, kernel
        assert paths == own.sum() * spec.launches[i][0]
        assert (paths, rays, shaded) == l_off[:3] and l_off[3] == 0
        if spec.oracle_tile == spec.tile:
            assert (paths, rays, shaded) == l_ref
        assert replays == want if exact else replays <= min(want, paths - own.sum())
    # against the oracle: the whole small frame (a tile share's other pixels are untouched on both sides), the oracle's tiles of the large one
    bad = np.argwhere((on[0] != ref[0]).any(axis=-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first {bad[0]}: gpu {on[0][tuple(bad[0])]} oracle {ref[0][tuple(bad[0])]}"
    assert np.array_equal(on[1], ref[1])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2] == off[2]
    if spec.tile[1] > 1:                # the other ranks' pixels: the cleared accumulator and the seeded texture
        assert own.any() and not own.all()
        assert not on[0][~own].any() and np.array_equal(on[1][~own], host.fill_rng(RSEED, spec.W, spec.H)[~own])
    return on


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_matrix_persistent_workgroups(rgpu, scene, env):
    """trimat::k_render_pwg<PATH>, k_render_pwg_tex<PATH> and its twin: material and uv through the 10-row memo, emitter triangles and
    escaping rays through its radiance rows, under a colour and under the map"""
    _verify(rgpu, Spec(scene, env))


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("scene", DENSE_SCENES)
def test_replay_matrix_dense(rgpu, scene, env):
    """trimat::k_render_dense: the packed word of the 7-row memo with a material per triangle; with checker cubes the cubes' pixels and
    those of the triangles that share their materials walk every sample"""
    spec = Spec(scene, env, DW, DH)
    on = _verify(rgpu, spec)
    if scene.endswith("checker") and on[3][0][5]["dense_memo_rows"] < 10:
        assert spec.hits(0)["uv_read"].sum() > 10000 and spec.hits(0)["uv_read"][spec.hits(0)["triangle"]].any()


@pytest.mark.parametrize("scene", DENSE_SCENES)
def test_replay_matrix_dense_keeps_the_side_of_a_hit(rgpu, scene):
    """from the far left the small ball shows triangles whose sn is -gn, thousands of pixels on a material the memo keeps: the side
    bit of the packed word (the matrix's own camera sees next to none on this ball)"""
    spec = Spec(scene, "rgb", DW, DH, launches=((SPP, 0, 2),))
    h = spec.hits(2)
    assert (h["back"] & ~h["emitter"] & ~h["uv_read"]).sum() > 1000 and (h["back"] & h["emitter"]).any()
    _verify(rgpu, spec)


@pytest.mark.parametrize("chain", [1, 3, 1 << 20])
@pytest.mark.parametrize("min_lanes", [1, 2, 33, 64, 65])
def test_replay_schedule_knobs_change_nothing(rgpu, min_lanes, chain):
    """replay_min_lanes x replay_chain on the three persistent-workgroup scenes: which trip of the loop shades a replayed hit is
    wave-uniform scheduling -- the same bits and the same count as the defaults give (65 lanes: no trip shades replayed hits alone)"""
    for scene in sorted(PWG_SCENES):
        spec = Spec(scene, "spiky" if scene == "trimat+tex" else "rgb")
        _same_run(_verify(rgpu, spec, min_lanes=min_lanes, chain=chain), _run(rgpu, spec))


@pytest.mark.parametrize("min_lanes,chain", [(1, 1), (64, 1), (65, 1), (1, 1 << 20)])
def test_replay_schedule_knobs_change_nothing_dense(rgpu, min_lanes, chain):
    spec = Spec("dense-trimat-checker", "rgb", DW, DH)
    _same_run(_verify(rgpu, spec, min_lanes=min_lanes, chain=chain), _run(rgpu, spec))


@pytest.mark.parametrize("min_lanes", [16, 17])
@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_in_blocks_of_sixteen_lanes(rgpu, scene, min_lanes):
    """TRC_FLAG_SMALL_BLOCKS: 4 x 4 pixels on 16 lanes -- 16 lanes can all hold a replayed hit, 17 never do"""
    on = _verify(rgpu, Spec(scene, small_blocks=True), min_lanes=min_lanes)
    _same_run(on, _run(rgpu, Spec(scene)))          # ... and the frame of the 8 x 8 blocks


@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_on_a_tile_share(rgpu, scene):
    """rank 1 of 3: the other ranks' pixels stay untouched, and only this rank's are counted"""
    _verify(rgpu, Spec(scene, tile=(1, 3)))


@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_in_stacked_views(rgpu, scene):
    """two views of 61 x 23 stacked in a frame of 61 x 46: the memo is the pixel's, v is the view's"""
    _verify(rgpu, Spec(scene, H=46, view_height=23))


@pytest.mark.parametrize("max_depth", [1, 2])
@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_with_short_paths(rgpu, scene, max_depth):
    _verify(rgpu, Spec(scene, "spiky", max_depth=max_depth))


@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_with_an_odd_sample_count(rgpu, scene):
    _verify(rgpu, Spec(scene, launches=((9, 0, 0),)))


@pytest.mark.parametrize("moved", [False, True], ids=["same-camera", "moved-camera"])
@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_continues_a_frame(rgpu, scene, moved):
    """a second launch onto the first's accumulator, frame0 continuing -- and the same with the camera moved in between: the memo
    never outlives its block, the second launch is the oracle's from the new eye"""
    _verify(rgpu, Spec(scene, launches=((SPP, 0, 0), (SPP, SPP, 1 if moved else 0))))


@pytest.mark.parametrize("scene", sorted(PWG_SCENES))
def test_replay_under_a_cold_head(rgpu, scene):
    """24 samples: a call that a cold head may split into passes, each with a first walk of its own -- the oracle's bits, and no
    more replays than one launch would count"""
    _verify(rgpu, Spec(scene, launches=((24, 0, 0),)), exact=False)


@pytest.mark.parametrize("scene", DENSE_SCENES)
def test_replay_in_split_parts_on_dense(rgpu, scene):
    """three consecutive launches of 8 samples: the second and third run the adaptive order and its split parts (quarters, sixteenths
    and single pixels of a block that ran long: few active lanes).  Every pixel is still in exactly one part of each launch."""
    _verify(rgpu, Spec(scene, "spiky", DW, DH, launches=((SPP, 0, 0), (SPP, SPP, 0), (SPP, 2 * SPP, 0))))
