"""trc_denoise_track_motion on the GPU (include/tracer_abi.h "Motion tracking", tracer_amd/csrc/trc_denoise.hip): the motion plane
against its definition (tests/motion_ref.py) over the production walk's hits, animated sequences plane by plane against the CPU
restatement (tests/svgf_motion_ref/svgf_motion_ref.cpp), that the history really survives a moving surface, and what the switch
leaves alone: a context that does not animate, a context with tracking off, every call that drops the history."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_motion_ref"))
import svgf_motion_loader as sml  # noqa: E402

import morph_ref as mref  # noqa: E402
import motion_ref as mr  # noqa: E402
import pose_ref as pr  # noqa: E402
import refit_ref as rr  # noqa: E402
import skin_ref as sr  # noqa: E402
from conftest import camera_rays  # noqa: E402
from test_gpu_update_vertices import DEVICE_TREE, scene  # noqa: E402
from test_svgf_ref import rotated  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer, TracerError  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"lds": (96, 64), "mem": (173, 97)}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sml.build(tmp_path_factory.mktemp("svgf_motion_ref_gpu"))


@pytest.fixture
def tracked():
    """a context of its own with the test hooks and tracking on (the session's contexts keep the default)"""
    with Tracer(0, hooks=True) as t:
        t.denoise_track_motion(True)
        yield t


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def setup(trc, residence, W, H, device_tree=False):
    if device_tree:
        trc.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    else:
        trc.upload_scene(scene(residence).view)
    trc.set_camera(host.prepare_camera(W, H))
    trc.set_environment((0.0, 0.0, 0.0))
    trc.resize(W, H)
    trc.seed(11)


def frame(trc, k, p=None):
    """one frame of an animated host: a fresh accumulator, 1 sample per pixel, trc_denoise"""
    trc.clear_accum()
    trc.render(spp=1, frame0=k, integrator=abi.INTEGRATOR_PATH)
    trc.denoise(p)


def centre(residence):
    return pr.box_centre(rr.vertices_of(scene(residence).view))


def n_vertex(residence):
    return scene(residence).view.n_vertex


def expected_motion(trc, cam, W, H, snapshot, residence):
    """tests/motion_ref.py over the production walk's hits of the G-buffer rays, the device's current vertices and `snapshot`"""
    hits = trc.trace_rays(camera_rays(cam, W, H), production=True)
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    o, d = mr.gbuffer_rays(cam, W, H)
    want = mr.texels(o, d, np.where(tri, hits["pIndex"].astype(np.int64), -1), trc.download_vertices(), snapshot,
                     rr.indices_of(scene(residence).view))
    return want.reshape(H, W), hits.reshape(H, W), tri.reshape(H, W)


def assert_motion(got, want, what):
    assert np.array_equal(got["moved"], want["moved"]), what
    bad = (bits(got["prev"]) != bits(want["prev"])).any(-1)
    assert not bad.any(), (what, int(bad.sum()), got["prev"][bad][:3], want["prev"][bad][:3])


# ----------------------------------------------------------------------------------------------------------- the moves
def do_pose(trc, residence, k, step_deg=5.0, shift=(0.0, 0.0, 0.0)):
    s = tuple(F(k) * F(c) for c in shift)
    trc.pose_vertices([(0, n_vertex(residence), *pr.turn(centre(residence), np.radians(step_deg * k), shift=s))])


def do_update(trc, residence, k):
    trc.update_vertices(rr.twist(rr.vertices_of(scene(residence).view), 0.15 * k, 1.0 - 0.02 * k))


def do_skin(trc, residence, k):
    if k == 1:
        trc.skin_bind(*sr.binding(n_vertex(residence), 4))
    trc.skin_vertices([pr.turn(centre(residence), 0.03 * k * (b + 1), shift=(2.0 * k * b, 0.0, 0.0)) for b in range(4)])


def do_morph(trc, residence, k):
    if k == 1:
        trc.morph_bind(mref.deltas(2, n_vertex(residence)))
    trc.morph_vertices(F([0.5 * k, -0.3 * k]))


MOVES = {"pose": do_pose, "update": do_update, "skin": do_skin, "morph": do_morph}


# ----------------------------------------------------------------------------------------------------------- the motion plane
# (a device-built tree runs the same kernels over another tree: two of the moves pin it)
PLANE_CASES = [(m, False) for m in ("pose", "update", "skin", "morph", "update_unchanged")] + [("pose", True), ("update_unchanged", True)]


@pytest.mark.parametrize("move,device_tree", PLANE_CASES)
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_motion_plane_is_the_definition_s(tracked, residence, move, device_tree):
    W, H = SIZES[residence]
    cam = host.prepare_camera(W, H)
    setup(tracked, residence, W, H, device_tree)
    frame(tracked, 0)
    assert not tracked.download_motion().view(np.uint32).any()          # no snapshot in force: all zero
    snapshot = tracked.download_vertices()
    if move == "update_unchanged":
        tracked.update_vertices(snapshot)
    else:
        MOVES[move](tracked, residence, 1)
    frame(tracked, 1)
    got = tracked.download_motion()
    want, hits, tri = expected_motion(tracked, cam, W, H, snapshot, residence)
    assert tri.sum() > 50
    assert_motion(got, want, (residence, move))
    if move == "update_unchanged":
        assert not got["moved"].any()
        assert np.array_equal(bits(got["prev"][tri]), bits(hits["p"][tri]))
    else:
        assert got["moved"][tri].all() and not got["moved"][~tri].any()
    g = tracked.download_gbuffer()                                       # the G-buffer beside it is the untracked kernel's
    assert np.array_equal(bits(g["depth"][hits["hit"] != 0]), bits(hits["t"][hits["hit"] != 0]))


# ----------------------------------------------------------------------------------------------------------- sequences, bit for bit
def run_sequence(trc, ref, residence, size, moves, cams=None, n_frames=6, p=None, device_tree=False):
    """moves(trc, k) animates in front of frame k >= 1 and returns whether a vertex moved (a snapshot is then in force).  Every frame:
    the motion plane against motion_ref, then integrated, history, moments and output against the restatement fed with that plane.
    -> per frame (moments, motion, gbuffer)"""
    W, H = size
    base = host.prepare_camera(W, H)
    setup(trc, residence, W, H, device_tree)
    p = p if p is not None else trc.denoise_params()
    rp = sml.params(**{f: getattr(p, f) for f, _ in p._fields_})
    ref.reset()
    frames = []
    for k in range(n_frames):
        cam = rotated(base, cams[k]) if cams else base
        trc.set_camera(cam)
        snapshot = trc.download_vertices()
        in_force = bool(moves(trc, k)) if k else False
        frame(trc, k, p)
        motion = trc.download_motion()
        if in_force:
            assert_motion(motion, expected_motion(trc, cam, W, H, snapshot, residence)[0], k)
        if not in_force:
            assert not motion.view(np.uint32).any(), k
        accum, g, out = trc.download_accum(), trc.download_gbuffer(), trc.download_denoised()
        integ, hist, mom = trc.denoise_state()
        r_integ, r_hist, r_mom, r_out = ref.frame(rp, sml.cam_vectors(cam), g, accum, motion if in_force else None)
        for what, a, b in (("integrated", integ, r_integ), ("history", hist, r_hist), ("moments", mom, r_mom), ("out", out, r_out)):
            bad = bits(a) != bits(b)
            assert not bad.any(), (f"{residence} frame {k}: {what} differs in {int(bad.any(-1).sum())} pixels", a[bad.any(-1)][:3], b[bad.any(-1)][:3])
        frames.append((mom, motion, g))
    return frames


def seq_pose(trc, res, k):
    do_pose(trc, res, k); return True


def seq_pose_shift(trc, res, k):
    do_pose(trc, res, k, shift=(25.0, 0.0, 0.0)); return True          # 25 units of the 555-unit box: 4 pixels of 96, 8 of 173


def seq_update(trc, res, k):
    do_update(trc, res, k); return True


def seq_skin(trc, res, k):
    do_skin(trc, res, k); return True


def seq_morph(trc, res, k):
    do_morph(trc, res, k); return True


def seq_pose_then_normals(trc, res, k):
    do_pose(trc, res, k); trc.recompute_normals(); return True          # the snapshot is the state before the pose


def seq_two_denoises_between_moves(trc, res, k):
    if k % 2 == 0:
        return False                                                    # nothing moved since the last trc_denoise: no snapshot
    do_pose(trc, res, (k + 1) // 2); return True


def seq_rebuild(trc, res, k):
    do_pose(trc, res, k); trc.rebuild_tree(abi.TREE_SAH if k % 2 else 0); return True


def seq_normals_only(trc, res, k):
    trc.recompute_normals(); return False                               # no vertex moved: history kept, no snapshot


SEQUENCES = [("pose", seq_pose, None, False), ("camera_and_pose", seq_pose, [0.5 * k for k in range(6)], False),
             ("pose_shift", seq_pose_shift, None, False), ("update", seq_update, None, False), ("skin", seq_skin, None, False),
             ("morph", seq_morph, None, False), ("pose_then_normals", seq_pose_then_normals, None, False),
             ("two_denoises_between_moves", seq_two_denoises_between_moves, None, False), ("rebuild_tree", seq_rebuild, None, True),
             ("normals_only", seq_normals_only, None, False)]


@pytest.mark.parametrize("name,moves,cams,device_tree", SEQUENCES, ids=[s[0] for s in SEQUENCES])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_animated_sequence_equals_restatement(tracked, ref, residence, name, moves, cams, device_tree):
    demod = name in ("camera_and_pose", "skin", "rebuild_tree")
    p = tracked.denoise_params(demodulate=demod, iterations=1 if name == "morph" else 5)
    frames = run_sequence(tracked, ref, residence, SIZES[residence], lambda t, k: moves(t, residence, k), cams, p=p, device_tree=device_tree)
    moved_any = any(f[1]["moved"].any() for f in frames)
    assert moved_any == (name != "normals_only")
    if name in ("two_denoises_between_moves", "normals_only"):
        assert (frames[-1][0][..., 2] > 2).any()                         # the history went on through the frames without a snapshot


# ----------------------------------------------------------------------------------------------------------- the history survives
def self_consistent(g):
    """hit pixels whose normal passes the filter's consistency test with itself (interpolated mesh normals need not be unit): the self
    test of tests/test_gpu_denoise.py's still-camera case"""
    n = g["normal"]
    return np.isfinite(g["depth"]) & ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2] >= F(0.9))


def test_history_survives_on_the_moving_ball_and_on_the_walls(tracked, ref):
    """the 50 x 50 ball turning 5 degrees per frame under a still camera, 96 x 64: of the moved pixels of the last frame at least 0.9
    have the full history, and every static pixel that saw the same material in every frame keeps counting.

    "The full history" of a moved pixel is the frame count up to the rounding of step 2: its n is N / W + 1 over FOUR taps, and the
    weighted mean of four equal lengths k is k exactly only where every w * k is exact (k a power of two); with k = 3 and 5 on the way
    to frame 6 it is not.  One frame is at most 12 binary32 roundings (4 products, 3 + 3 additions, the division, the + 1) of values
    <= 6, five frames follow the first: |n - 6| <= 5 * 12 * 6 * 2^-24 = 2.1e-5.  Measured (the restatement on the CPU oracle's hit
    records, which the device equals bit for bit, and on an MI355X): 0.936 of 361 moved pixels within that bound at 5 degrees, 0.806
    of them with the bits of 6.0 -- and no angle brings bitwise equality to 0.9 (2 degrees 0.869, 1 degree 0.841, 0.5 degrees 0.852):
    what is left is rounding, not lost history (0.978 are above 5, 0.003 are at 1)"""
    n_frames = 6
    frames = run_sequence(tracked, ref, "mem", (96, 64), lambda t, k: seq_pose(t, "mem", k), n_frames=n_frames)
    mom, motion, g = frames[-1]
    moved = motion["moved"] == 1
    n = mom[..., 2][moved]
    full = np.abs(n - F(n_frames)) <= 5 * 12 * n_frames * 2.0 ** -24
    print(f"moved pixels {int(moved.sum())}, with history {n_frames}: {full.mean():.4f} up to rounding, {(n == F(n_frames)).mean():.4f} bitwise")
    assert moved.sum() > 100 and full.mean() >= 0.9
    static = np.isfinite(g["depth"]) & ~moved & self_consistent(g)
    for _, _, gk in frames[:-1]:                                         # the same surface at that pixel in every earlier frame
        static &= gk["id"] == g["id"]
    for _, mk, _ in frames:
        static &= mk["moved"] == 0
    assert static.sum() > 1000 and np.all(mom[..., 2][static] == F(n_frames))


# ----------------------------------------------------------------------------------------------------------- what stays as it was
def planes(trc):
    return (trc.download_accum(), trc.download_gbuffer(), trc.download_denoised()) + trc.denoise_state()


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_tracking_on_with_nothing_moved_changes_no_bit(residence):
    W, H = SIZES[residence]
    base = host.prepare_camera(W, H)
    with Tracer(0, hooks=True) as on, Tracer(0, hooks=True) as off:
        on.denoise_track_motion(True)
        for t in (on, off):
            setup(t, residence, W, H)
        for k in range(5):
            for t in (on, off):
                t.set_camera(rotated(base, 0.5 * (k // 2)))             # still, a step, still
                frame(t, k, t.denoise_params(demodulate=True))
            for a, b in zip(planes(on), planes(off)):
                assert a.tobytes() == b.tobytes(), k
            assert not on.download_motion().view(np.uint32).any()
        assert (on.denoise_state()[2][..., 2] > 1).any()


def history(trc):
    g = trc.download_gbuffer()
    return trc.denoise_state()[2][..., 2][np.isfinite(g["depth"])]


@pytest.mark.parametrize("move", ["pose", "update", "skin", "morph", "recompute_normals", "rebuild_tree"])
def test_tracking_off_an_animation_call_still_drops_the_history(gpu_hooks, move):
    W, H = 64, 48
    setup(gpu_hooks, "lds", W, H, device_tree=move == "rebuild_tree")
    for k in range(3):
        frame(gpu_hooks, k)
    assert np.all(gpu_hooks.denoise_state()[2][..., 2][self_consistent(gpu_hooks.download_gbuffer())] == 3.0)
    if move == "recompute_normals":
        gpu_hooks.recompute_normals()
    elif move == "rebuild_tree":
        gpu_hooks.rebuild_tree(abi.TREE_SAH)
    else:
        MOVES[move](gpu_hooks, "lds", 1)
    frame(gpu_hooks, 3)
    assert np.all(history(gpu_hooks) == 1.0)
    with pytest.raises(TracerError) as e:
        gpu_hooks.download_motion()
    assert e.value.status == abi.ERR_NO_FRAME


TRIGGERS = ["resize", "upload_scene", "upload_scene_lbvh", "set_environment", "set_environment_map", "denoise_reset",
            "upload_textures", "upload_triangle_materials", "tracking_off_and_on", "tracking_off"]


@pytest.mark.parametrize("trigger", TRIGGERS)
def test_tracking_on_every_reset_trigger_still_drops_the_history(tracked, trigger):
    W, H = 64, 48
    sc = scene("lds")
    setup(tracked, "lds", W, H)
    for k in range(3):
        if k:
            do_pose(tracked, "lds", k)
        frame(tracked, k)
    assert (history(tracked) == 3.0).mean() > 0.5                       # the history did survive the poses
    do_pose(tracked, "lds", 3)                                          # a snapshot is in force when the trigger comes
    if trigger == "resize":
        tracked.resize(W, H); tracked.seed(1)
    elif trigger == "upload_scene":
        tracked.upload_scene(sc.view)
    elif trigger == "upload_scene_lbvh":
        tracked.upload_scene_lbvh(sc.leaves_view())
    elif trigger == "set_environment":
        tracked.set_environment((0.0, 0.0, 0.0))
    elif trigger == "set_environment_map":
        tracked.set_environment_map(None)
    elif trigger == "upload_textures":
        tracked.upload_textures([np.full((2, 2, 3), 0.5, F)])
    elif trigger == "upload_triangle_materials":
        tracked.upload_triangle_materials(np.full(sc.view.n_index // 3, 4, np.uint32))
    elif trigger == "tracking_off_and_on":
        tracked.denoise_track_motion(False); tracked.denoise_track_motion(True)
    elif trigger == "tracking_off":
        tracked.denoise_track_motion(False)
    else:
        tracked.denoise_reset()
    frame(tracked, 3)
    assert np.all(history(tracked) == 1.0)
    if trigger == "tracking_off":
        with pytest.raises(TracerError) as e:
            tracked.download_motion()
        assert e.value.status == abi.ERR_NO_FRAME
        return
    # the switch survived: the next pose is followed again
    assert tracked.download_motion().shape == (H, W)
    do_pose(tracked, "lds", 1)
    frame(tracked, 4)
    m = tracked.download_motion()
    assert m["moved"].any() and (tracked.denoise_state()[2][..., 2][m["moved"] == 1] == 2.0).any()
    if trigger == "upload_triangle_materials":
        tracked.upload_triangle_materials(None)
    if trigger == "upload_textures":
        tracked.upload_textures([])


def test_history_length_read_back_is_the_moments_plane_s(tracked):
    setup(tracked, "lds", 64, 48)
    with pytest.raises(TracerError) as e:
        tracked.download_history_length()
    assert e.value.status == abi.ERR_NO_FRAME
    for k in range(3):
        if k:
            do_pose(tracked, "lds", k)
        frame(tracked, k)
    n = tracked.download_history_length()
    assert np.array_equal(bits(n), bits(tracked.denoise_state()[2][..., 2])) and (n > 1).any()
    assert tracked._L.trc_download_history_length(tracked._h, None) == abi.ERR_INVALID_ARG


def test_error_codes():
    with Tracer(0) as t:
        NULL = None
        assert t._L.trc_denoise_track_motion(NULL, 1) == abi.ERR_INVALID_ARG
        assert t._L.trc_download_motion(NULL, NULL) == abi.ERR_INVALID_ARG
        assert t._L.trc_download_motion(t._h, NULL) == abi.ERR_INVALID_ARG
        W, H = 32, 32
        buf = np.zeros((H, W), mr.MOTION)

        def status():
            return t._L.trc_download_motion(t._h, buf.ctypes.data)
        assert status() == abi.ERR_NO_FRAME                              # tracking off, no frame
        t.denoise_track_motion(True)
        assert status() == abi.ERR_NO_FRAME                              # no frame
        setup(t, "lds", W, H)
        assert status() == abi.ERR_NO_FRAME                              # no trc_denoise yet
        t.denoise_track_motion(False)
        t.denoise()
        assert status() == abi.ERR_NO_FRAME                              # a trc_denoise, but tracking is off
        t.denoise_track_motion(True)
        assert status() == abi.ERR_NO_FRAME                              # ... and none since it is on
        t.denoise()
        assert status() == abi.OK and not buf.view(np.uint32).any()
        t.denoise_track_motion(True)                                     # the switch as it stands: nothing happens
        assert status() == abi.OK
        with pytest.raises(TracerError) as e:                            # tracking is no flag of trc_denoise_params
            t.denoise(flags=2)
        assert e.value.status == abi.ERR_INVALID_ARG
        t.resize(W, H)                                                   # the plane goes with the frame, the switch stays
        assert status() == abi.ERR_NO_FRAME
        t.denoise()
        assert status() == abi.OK
        t.denoise_track_motion(False)
        assert status() == abi.ERR_NO_FRAME


# ----------------------------------------------------------------------------------------------------------- quality
# Measured on an MI355X (profiles/r24/denoise_motion.txt): RMSE of frame 8 against 2048 spp over the whole frame 0.18427 tracked,
# 0.19174 untracked; over the 810 moved pixels 0.01313 tracked, 0.01322 untracked (the ball is dark beside the lamp's fireflies, which
# carry the whole-frame figure).  The assertion is the strict inequality alone, over the whole frame.
def test_tracking_lowers_the_error_of_an_animated_sequence():
    """the 50 x 50 ball, 8 frames of a 5-degree pose at 160 x 96, against 2048 samples of the last pose: the tracked run's last frame is
    closer to the truth than the same sequence with tracking off (every frame of which starts at history 1: the parent's behaviour)"""
    W, H, n_frames = 160, 96, 8
    rmse = lambda a, b, sel: float(np.sqrt(np.mean((a[sel][..., :3].astype(np.float64) - b[sel][..., :3].astype(np.float64)) ** 2)))
    outs = {}
    with Tracer(0) as t:
        for on in (True, False):
            t.denoise_track_motion(on)
            setup(t, "mem", W, H)
            t.seed(5)
            for k in range(n_frames):
                if k:
                    do_pose(t, "mem", k)
                frame(t, k)
            outs[on] = t.download_denoised()
            if on:
                moved = t.download_motion()["moved"] == 1
        t.seed(1234); t.clear_accum()
        t.render(spp=2048)
        truth = t.download_accum()
    everywhere = np.ones((H, W), bool)
    e = {on: (rmse(outs[on], truth, everywhere), rmse(outs[on], truth, moved)) for on in (True, False)}
    print(f"RMSE against 2048 spp, frame {n_frames}: tracked {e[True][0]:.5f} (moved pixels {e[True][1]:.5f}), "
          f"untracked {e[False][0]:.5f} (moved pixels {e[False][1]:.5f}); moved pixels {int(moved.sum())}")
    assert e[True][0] < e[False][0]


def test_fast_math_build_agrees_statistically():
    """libtracer_amd_fast.so: the denoised tracked frame of the same accumulators agrees with the exact build's to the 1e-3 relative RMS
    of tests/test_gpu_denoise.py's fast-math case"""
    W, H = 160, 96
    outs, accs = [], []
    for fast in (False, True):
        with Tracer(0, fast_math=fast) as t:
            t.denoise_track_motion(True)
            setup(t, "mem", W, H)
            for k in range(3):
                if k:
                    do_pose(t, "mem", k)
                if not fast:
                    t.clear_accum(); t.render(spp=1, frame0=k)
                    accs.append(t.download_accum())
                t.upload_accum(accs[k])
                t.denoise(t.denoise_params(demodulate=True))
            assert (t.download_motion()["moved"] == 1).sum() > 100
            outs.append(t.download_denoised()[..., :3].astype(np.float64))
    rel = np.sqrt(np.mean((outs[0] - outs[1]) ** 2)) / np.sqrt(np.mean(outs[0] ** 2))
    assert rel < 1e-3, rel
