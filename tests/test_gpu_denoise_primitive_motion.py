"""trc_denoise_track_motion behind trc_update_primitives on the GPU (include/tracer_abi.h "Motion tracking"): the motion texels of
sphere, square and cube winners against their definition (tests/primitives_ref.py) beside the triangle rule (tests/motion_ref.py), over
the production walk's hits; a sequence that moves both kinds of geometry plane by plane against the CPU restatement
(tests/svgf_motion_ref); the history on the walls and on a moving sphere; what tracking leaves alone; the example host's --orbit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_motion_ref"))
import svgf_motion_loader as sml  # noqa: E402

import motion_ref as mr  # noqa: E402
import pose_ref as por  # noqa: E402
import primitives_ref as pr  # noqa: E402
import refit_ref as rr  # noqa: E402
from conftest import camera_rays  # noqa: E402
from test_gpu_denoise_motion import assert_motion, bits, frame, planes  # noqa: E402
from test_gpu_update_vertices import scene  # noqa: E402
from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 32
_SCENES = {}


class Both:
    """Cornell + the 48-triangle ball WITH its twelve spheres in the tree: the mesh scene's leaves and a leaf per sphere under
    trc_host_build_tree, so that one scene has moving spheres, cubes, squares and triangles"""

    def __init__(self):
        self.base = scene("lds")
        v = self.base.view
        leaves = [self.base.leaves()[i] for i in range(self.base.n_leaves)]
        for k, s in enumerate(pr.spheres_of(v)):
            b = s.boundingBOX
            leaves.append(host.build_node((b.mini.x, b.mini.y, b.mini.z), (b.maxi.x, b.maxi.y, b.maxi.z), abi.PRIM_SPHERE, k))
        self.nodes = host.build_tree(leaves)
        self.view = self.base.view_with_bvh(self.nodes)


def scn(name):
    if name not in _SCENES:
        _SCENES[name] = host.HostScene(abi.SCENE_CORNELL_SPHERES) if name == "spheres" else Both() if name == "both" else scene(name)
    return _SCENES[name]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sml.build(tmp_path_factory.mktemp("svgf_primitive_motion_ref_gpu"))


@pytest.fixture
def tracked():
    with Tracer(0, hooks=True) as t:
        t.denoise_track_motion(True)
        yield t


def setup(trc, name, lbvh=False):
    sc = scn(name)
    if lbvh:
        trc.upload_scene_lbvh(sc.leaves_view())
    else:
        trc.upload_scene(sc.view)
    trc.set_camera(host.prepare_camera(W, H))
    trc.set_environment((0.0, 0.0, 0.0))
    trc.resize(W, H)
    trc.seed(11)


def orbit(view, k, cube=False, square=False):
    """the scene's lists with every sphere 9 degrees * k round the vertical axis through the middle of the box; cube: cube 0 turned and
    shifted; square: the light square shifted and shrunk"""
    sp, sq, cb = pr.motion(view, 0.0)
    a = np.radians(9.0 * k)
    for i in range(len(sp)):
        c, r = sp[i].center, F(sp[i].radius) - F(0.0001)
        x, z = c.x - 278.0, c.z - 278.0
        sp[i] = host.make_sphere(r, (F(278.0 + np.cos(a) * x + np.sin(a) * z), c.y, F(278.0 - np.sin(a) * x + np.cos(a) * z)), sp[i].material)
    if cube:
        cb[0] = host.make_cube(cb[0].material, pr.rotation_y(0.26 + 0.12 * k, (265 + 6 * k, 1, 295), (165, 330, 165)))
    if square:
        s = sq[5]
        sq[5] = host.make_square(s.axis_i, F(s.range_i.x - 20 * k), F(s.range_i.y - 30 * k), s.axis_j, s.range_j.x, F(s.range_j.y - 10 * k), s.axis_k, s.value_k, s.material)
    return sp, sq, cb


def update(trc, lists):
    trc.update_primitives(spheres=lists[0], squares=lists[1], cubes=lists[2])


def expected_motion(trc, name, cam, now, then, vertices_then):
    """motion_ref on triangle winners, primitives_ref on analytic winners, over the production walk's hits of the G-buffer rays"""
    view = scn(name).view
    hits = trc.trace_rays(camera_rays(cam, W, H), production=True)
    want = pr.motion_texels(hits, now, then)
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    if view.n_vertex:
        o, d = mr.gbuffer_rays(cam, W, H)
        t = mr.texels(o, d, np.where(tri, hits["pIndex"].astype(np.int64), -1), trc.download_vertices(), vertices_then, rr.indices_of(view))
        want[tri] = t[tri]
    return want.reshape(H, W), hits.reshape(H, W)


# ----------------------------------------------------------------------------------------------------------- 1. the motion plane
@pytest.mark.parametrize("name,lbvh", [("spheres", False), ("spheres", True), ("mem", False), ("both", False)])
def test_motion_plane_is_the_definition_s(tracked, name, lbvh):
    view = scn(name).view
    cam = host.prepare_camera(W, H)
    setup(tracked, name, lbvh)
    frame(tracked, 0)
    assert not tracked.download_motion().view(np.uint32).any()          # no snapshot in force: all zero
    then = pr.motion(view, 0.0)
    vertices_then = tracked.download_vertices() if view.n_vertex else None
    now = orbit(view, 1, cube=True, square=True)
    update(tracked, now)
    frame(tracked, 1)
    got = tracked.download_motion()
    want, hits = expected_motion(tracked, name, cam, now, then, vertices_then)
    assert_motion(got, want, name)
    hit = hits["hit"] != 0
    kinds = {t: hit & (hits["pType"] == t) for t in (abi.PRIM_SPHERE, abi.PRIM_SQUARE, abi.PRIM_CUBE, abi.PRIM_TRIANGLE)}
    assert got["moved"][kinds[abi.PRIM_CUBE] & (hits["pIndex"] == 0)].all() and (kinds[abi.PRIM_CUBE] & (hits["pIndex"] == 0)).sum() > 10
    light = kinds[abi.PRIM_SQUARE] & (hits["pIndex"] == 5)
    assert light.any() and got["moved"][light].all()
    assert not got["moved"][kinds[abi.PRIM_SQUARE] & (hits["pIndex"] != 5)].any()      # the walls stand
    if name != "mem":                                                                   # (the mesh scene's tree holds no sphere)
        assert kinds[abi.PRIM_SPHERE].sum() > 20 and got["moved"][kinds[abi.PRIM_SPHERE]].all()
    if view.n_vertex:                                                                   # one snapshot for both kinds: the ball stood
        assert kinds[abi.PRIM_TRIANGLE].any() and not got["moved"][kinds[abi.PRIM_TRIANGLE]].any()
        assert np.array_equal(bits(got["prev"][kinds[abi.PRIM_TRIANGLE]]), bits(hits["p"][kinds[abi.PRIM_TRIANGLE]]))
    g = tracked.download_gbuffer()                                       # the G-buffer beside it is the untracked kernel's
    assert np.array_equal(bits(g["depth"][hit]), bits(hits["t"][hit]))


def test_unchanged_records_move_nothing(tracked):
    """the scene's own records sent again: a snapshot is in force, every compare finds equal bits, the history goes on"""
    view = scn("spheres").view
    setup(tracked, "spheres")
    for k in range(2):
        frame(tracked, k)
    update(tracked, pr.motion(view, 0.0))
    frame(tracked, 2)
    assert not tracked.download_motion().view(np.uint32).any()
    n = tracked.download_history_length()
    assert (n == 3.0).sum() > 0.5 * W * H


# ----------------------------------------------------------------------------------------------------------- 2. a sequence, bit for bit
def run_sequence(trc, ref, n_frames=6):
    """frames 1..5 of 'both': spheres orbit; the cube turns; the ball is posed; spheres, then a pose; a pose, then the cube.  Every
    frame's motion plane against the definitions, then every plane of the filter against the restatement fed with that plane"""
    name = "both"
    view = scn(name).view
    cam = host.prepare_camera(W, H)
    setup(trc, name)
    p = trc.denoise_params(demodulate=True)
    rp = sml.params(**{f: getattr(p, f) for f, _ in p._fields_})
    ref.reset()
    v0 = rr.vertices_of(view)
    n = len(v0)
    lists = pr.motion(view, 0.0)
    frames = []

    def pose(k):
        trc.pose_vertices([(0, n, *por.turn(por.box_centre(v0), np.radians(6.0 * k)))])
    for k in range(n_frames):
        then, vertices_then = lists, trc.download_vertices()
        if k in (1, 4):
            lists = orbit(view, k)
            update(trc, lists)
        if k in (3, 4, 5):
            pose(k)
        if k in (2, 5):
            lists = orbit(view, 4 if k == 5 else 1, cube=True)
            trc.update_primitives(cubes=lists[2][:1])
        frame(trc, k, p)
        motion = trc.download_motion()
        if k:
            want, hits = expected_motion(trc, name, cam, lists, then, vertices_then)
            assert_motion(motion, want, k)
            assert motion["moved"].any(), k
        else:
            assert not motion.view(np.uint32).any()
        accum, g, out = trc.download_accum(), trc.download_gbuffer(), trc.download_denoised()
        integ, hist, mom = trc.denoise_state()
        r_integ, r_hist, r_mom, r_out = ref.frame(rp, sml.cam_vectors(cam), g, accum, motion if k else None)
        for what, a, b in (("integrated", integ, r_integ), ("history", hist, r_hist), ("moments", mom, r_mom), ("out", out, r_out)):
            bad = bits(a) != bits(b)
            assert not bad.any(), (f"frame {k}: {what} differs in {int(bad.any(-1).sum())} pixels", a[bad.any(-1)][:3], b[bad.any(-1)][:3])
        frames.append((mom, motion, g, trc.trace_rays(camera_rays(cam, W, H), production=True).reshape(H, W)))
    return frames


def test_sequence_of_both_kinds_equals_restatement(tracked, ref):
    frames = run_sequence(tracked, ref)
    kinds = set()
    for mom, motion, g, hits in frames[1:]:
        kinds |= set(int(t) for t in hits["pType"][(motion["moved"] == 1)])
    assert kinds == {abi.PRIM_SPHERE, abi.PRIM_CUBE, abi.PRIM_TRIANGLE}


# ----------------------------------------------------------------------------------------------------------- 3. the history
def test_history_on_the_walls_and_on_a_moving_sphere(tracked, ref):
    """Sphere 0 slides 2 units per frame along x under a still camera: a tenth of a pixel of the 48-pixel frame (the box is 1045 units
    wide in it).  A wall pixel whose primary hit never moved has history min(k, 64) after k frames, exactly (one tap under the same
    camera, weight 1: n = n' / 1 + 1 in integers).  A pixel that shows the moving sphere in two consecutive frames reprojects to within
    a tenth of a pixel of itself, so the tap of the greatest weight (>= 0.8) is that same pixel, which showed the sphere at nearly the
    same point: it has found its history, n > 1.  (At 9 degrees of orbit per frame, most of a pixel, 91 of 99 such pixels keep theirs on an
    MI355X, as the restatement says bit for bit: the silhouette's taps fall off the sphere.)  Every n is the restatement's, compared bit
    for bit frame by frame; with tracking off it is 1 everywhere after the call."""
    name = "spheres"
    view = scn(name).view
    cam = host.prepare_camera(W, H)
    setup(tracked, name)
    p = tracked.denoise_params()
    rp = sml.params(**{f: getattr(p, f) for f, _ in p._fields_})
    ref.reset()
    rays = camera_rays(cam, W, H)
    n_frames = 5
    never_moved = np.ones((H, W), bool)
    ids = before = None
    for k in range(n_frames):
        if k:
            s0 = pr.spheres_of(view)[0]
            tracked.update_primitives(spheres=[host.make_sphere(64.0, (s0.center.x + 2.0 * k, s0.center.y, s0.center.z), s0.material)])
        frame(tracked, k, p)
        motion, g, accum = tracked.download_motion(), tracked.download_gbuffer(), tracked.download_accum()
        mom = tracked.denoise_state()[2]
        r_mom = ref.frame(rp, sml.cam_vectors(cam), g, accum, motion if k else None)[2]
        assert np.array_equal(bits(mom), bits(r_mom)), k
        hits = tracked.trace_rays(rays, production=True).reshape(H, W)
        before, ids = ids, np.where(hits["hit"] != 0, hits["pType"].astype(np.int64) * 1000 + hits["pIndex"], -1)
        never_moved &= (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_SQUARE) & (motion["moved"] == 0)
        if before is not None:
            never_moved &= ids == before
    n = tracked.download_history_length()
    assert never_moved.sum() > 300 and np.all(n[never_moved] == F(min(n_frames, 64)))
    sphere = (ids == abi.PRIM_SPHERE * 1000) & (before == ids)           # sphere 0 in the last frame and in the one before
    print(f"pixels that show the moving sphere in both frames {int(sphere.sum())}, of those with n > 1: {int((n[sphere] > 1).sum())}, "
          f"with n = {n_frames}: {int((n[sphere] == n_frames).sum())}")
    # (the sphere's radius is 2.9 pixels here, 27 pixels of area: at least half of them show it twice)
    assert sphere.sum() >= 13 and (motion["moved"][sphere] == 1).all() and np.all(n[sphere] > 1)
    with Tracer(0) as off:
        setup(off, name)
        for k in range(3):
            frame(off, k)
        update(off, orbit(view, 1))
        frame(off, 3)
        assert np.all(off.download_history_length() == 1.0)                 # tracking off: the call drops the history


# ----------------------------------------------------------------------------------------------------------- 4. what stays as it was
def test_tracking_on_with_nothing_moved_changes_no_bit():
    with Tracer(0, hooks=True) as on, Tracer(0, hooks=True) as off:
        on.denoise_track_motion(True)
        for t in (on, off):
            setup(t, "spheres")
        for k in range(4):
            for t in (on, off):
                frame(t, k, t.denoise_params(demodulate=True))
            for a, b in zip(planes(on), planes(off)):
                assert a.tobytes() == b.tobytes(), k
            assert not on.download_motion().view(np.uint32).any()
        assert (on.denoise_state()[2][..., 2] > 1).any()


# ----------------------------------------------------------------------------------------------------------- 5. the example host
def test_example_host_orbit(tmp_path):
    exe = os.path.join(ROOT, "examples", "trc_render")
    assert os.path.exists(exe), "examples/trc_render is missing: run `make example`"
    out = tmp_path / "orbit.png"
    cmd = ["timeout", "-k", "10", "120", exe, "--scene", "spheres", "--size", "48", "32", "--spp", "2", "--orbit", "3", "--denoise", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("orbit ")]
    assert len(lines) == 3 and all("trc_update_primitives" in l and "mean history length" in l for l in lines), r.stdout
    lengths = [float(l.split("mean history length")[1].split()[0]) for l in lines]
    assert lengths[0] > 1.5 and lengths[2] > lengths[0]                  # the history is kept and grows (frame 0 left 1 everywhere)
    for k in (1, 2, 3):
        assert os.path.getsize(f"{out}.{k}.png") > 0
