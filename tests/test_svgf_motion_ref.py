"""The CPU side of trc_denoise_track_motion (include/tracer_abi.h, "Motion tracking"): the restatement of the amended SVGF stage
(tests/svgf_motion_ref/svgf_motion_ref.cpp) against the restatement without the amendment and on a surface that slides under a still
camera, and the restated motion texel (tests/motion_ref.py) against the CPU oracle's hit points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_ref"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_motion_ref"))
import svgf_loader as sl  # noqa: E402
import svgf_motion_loader as sml  # noqa: E402

import motion_ref as mr  # noqa: E402
from conftest import camera_rays  # noqa: E402
from test_svgf_ref import noisy, plane_gbuffer, rotated  # noqa: E402
from tracer_amd import abi, host  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("svgf_motion_ref")
    return sl.build(d), sml.build(d)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------- nothing moved: the stage as it was
@pytest.mark.parametrize("plane", ["none", "zero", "prev_without_moved"])
@pytest.mark.parametrize("demod,iters", [(False, 5), (True, 5), (True, 1), (False, 0)])
def test_zero_motion_plane_is_the_existing_restatement_bit_for_bit(refs, demod, iters, plane):
    """the sequences of tests/test_svgf_ref.py: a still camera, one stepping 0.5 degrees, a jump; a depth step and a block of misses.
    A texel with moved = 0 takes step 2 as it stands whatever its prev holds"""
    old, new = refs
    W, H = 64, 40
    base = host.prepare_camera(W, H)
    views = [0.0, 0.0, 0.5, 1.0, 1.5, 1.5, 1.5, 4.0]
    p = sl.params(demodulate=demod, iterations=iters)
    old.reset(); new.reset()
    for k, deg in enumerate(views):
        cam = rotated(base, deg)
        g = plane_gbuffer(cam, W, H, step=(40, 2000.0) if k >= 3 else None)
        if k >= 5:
            g["depth"][8:16, 10:30] = np.inf; g["normal"][8:16, 10:30] = 0; g["albedo"][8:16, 10:30] = 1; g["id"][8:16, 10:30] = sl.MISS
        a = noisy(H, W, 100 + k)
        motion = None
        if plane != "none":
            motion = np.zeros((H, W), sml.MOTION)
            if plane == "prev_without_moved":
                motion["prev"] = np.random.default_rng(k).random((H, W, 3)) * 500.0
        want = old.frame(p, sl.cam_vectors(cam), g, a)
        got = new.frame(p, sl.cam_vectors(cam), g, a, motion)
        for what, x, y in zip(("integrated", "history", "moments", "out"), got, want):
            assert np.array_equal(bits(x), bits(y)), (k, what)
    assert (got[2][..., 2] > 1).any()


# ------------------------------------------------------------------------------------------------- a surface that slides
def sliding_plane(W, H, k_px, n_frames, tracked):
    """A fronto-parallel plane 600 in front of a still camera, carrying a luminance ramp, that slides k_px pixels to the right per
    frame.  -> per frame (g, accum, motion): motion says where each pixel's surface point was one frame earlier (the point pixel
    (x - k_px, y) sees), moved = 1 when `tracked`"""
    cam = host.prepare_camera(W, H)
    g = plane_gbuffer(cam, W, H, tilt=0.0)
    g["albedo"] = 0.5
    f = lambda a: np.array([a.x, a.y, a.z], np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    xs_src = xs - k_px
    d = f(cam.cornerLowLeft) + f(cam.horizontal) * (xs_src / W)[..., None] + f(cam.vertical) * (ys / H)[..., None] - f(cam.lookFrom)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    w = f(host.prepare_camera(W, H).w)
    w /= np.linalg.norm(w)
    t = 600.0 / -(d @ w)                          # the plane of plane_gbuffer(tilt=0): through lookFrom - 600 w, normal w
    prev = f(cam.lookFrom) + d * t[..., None]
    frames = []
    for k in range(n_frames):
        a = np.zeros((H, W, 4), F)
        a[..., :3] = (0.2 + 0.01 * (xs - k_px * k))[..., None]
        a[..., 3] = 1.0
        m = np.zeros((H, W), sml.MOTION)
        m["prev"] = prev
        m["moved"] = 1 if tracked else 0
        frames.append((g, a, m))
    return cam, frames


def test_history_follows_a_plane_that_slides_by_whole_pixels(refs):
    _, new = refs
    W, H, k_px, n_frames = 64, 24, 3, 6
    p = sml.params(iterations=0)
    cam, frames = sliding_plane(W, H, k_px, n_frames, tracked=True)
    # the plane really is where plane_gbuffer puts it: prev of a pixel is on the ray of the pixel k_px to its left, at that depth
    g0 = frames[0][0]
    eye = np.array([cam.lookFrom.x, cam.lookFrom.y, cam.lookFrom.z])
    dist = np.linalg.norm(frames[0][2]["prev"].astype(np.float64) - eye, axis=-1)
    np.testing.assert_allclose(dist[:, k_px:], g0["depth"][:, :-k_px], rtol=1e-5)
    new.reset()
    xs = np.mgrid[0:H, 0:W][1]
    for k, (g, a, m) in enumerate(frames, start=1):
        integ, _, mom, _ = new.frame(p, sml.cam_vectors(cam), g, a, m)
        # pixel x's chain of sources x - k_px, x - 2 k_px ... stays in bounds for min(k, x // k_px + 1) frames.  The reprojected tap
        # position is a whole pixel up to the float32 error of step 2's cancelling sums (1e-4 pixels, tests/test_svgf_ref.py), so a
        # neighbour tap whose history is up to k shorter enters with weight <= 1e-4: |n - expected| <= 1e-4 k, asserted as 1e-2
        expect = np.minimum(k, xs // k_px + 1).astype(F)
        assert np.abs(mom[..., 2] - expect).max() <= 1e-2, k
        # ... and the colour it integrates is the ramp it carries: the same neighbour taps differ by one step of the ramp (0.01)
        assert np.abs(integ[..., :3] - a[..., :3]).max() <= 1e-5, k
    assert np.all(np.abs(mom[:, (n_frames - 1) * k_px:, 2] - n_frames) <= 1e-2)


def test_history_smears_a_sliding_plane_without_the_motion_texel(refs):
    """moved = 0 under a still camera is the one tap at the same pixel: the history is another surface point's, 3 pixels of ramp away"""
    _, new = refs
    W, H, k_px, n_frames = 64, 24, 3, 6
    p = sml.params(iterations=0)
    cam, frames = sliding_plane(W, H, k_px, n_frames, tracked=False)
    new.reset()
    for k, (g, a, m) in enumerate(frames, start=1):
        integ, _, mom, _ = new.frame(p, sml.cam_vectors(cam), g, a, m)
        assert np.all(mom[..., 2] == F(k))
    # frame k blends c_k = c_{k-1} - 0.03 into the history with a = max(1 / k, 0.1): after 6 frames the lag is 0.03 * (5/6 + 4/6 ... )
    lag = integ[..., 0] - a[..., 0]
    assert lag.min() > 0.03


# ------------------------------------------------------------------------------------------------- the motion texel against the oracle
_SCENES = {}


def ball_scene(residence):
    """the scenes of tests/test_gpu_update_vertices.py: Cornell + a 48-triangle ball, Cornell + a 50 x 50 ball"""
    if residence not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.ball(50, 50, 0.08)
        _SCENES[residence] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
    return _SCENES[residence]


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_prev_of_an_unmoved_triangle_is_the_oracle_s_hit_point(residence):
    from oracle import pyoracle
    import refit_ref as rr
    W, H = 96, 64
    view = ball_scene(residence).view
    cam = host.prepare_camera(W, H)
    hits = pyoracle.trace_rays(view, camera_rays(cam, W, H))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 100
    v = rr.vertices_of(view)
    o, d = mr.gbuffer_rays(cam, W, H)
    m = mr.texels(o, d, np.where(tri, hits["pIndex"].astype(np.int64), -1), v, v, rr.indices_of(view))
    assert np.array_equal(bits(m["prev"][tri]), bits(hits["p"][tri]))
    assert not m["moved"].any() and not m["prev"][~tri].any()
    # ... and a snapshot that differs in one coordinate of one vertex marks exactly the triangles that name it
    idx = rr.indices_of(view)
    t0 = int(hits["pIndex"][tri][0])
    snap = v.copy()
    snap[idx[3 * t0 + 1], 2] += F(0.5)
    m2 = mr.texels(o, d, np.where(tri, hits["pIndex"].astype(np.int64), -1), v, snap, idx)
    names = (idx.reshape(-1, 3) == idx[3 * t0 + 1]).any(axis=1)
    want = tri & names[np.where(tri, hits["pIndex"], 0)]
    assert np.array_equal(m2["moved"] == 1, want) and want.any()
    assert np.array_equal(bits(m2["prev"][tri & ~want]), bits(hits["p"][tri & ~want]))
