"""trc_pose_vertices on the CPU: the ABI names it without a new version number, the definition (tests/pose_ref.py) can be told from
its near misses with the matrices the GPU tests use, and a tree refitted around posed vertices bounds them."""
import ctypes as C

import numpy as np

import pose_ref as pr
import refit_ref as rr
from conftest import random_rays
from oracle import pyoracle
from tracer_amd import abi, host

F = np.float32
# the poses of tests/test_gpu_pose_vertices.py: angles with inexact float32 cosine and sine, a non-uniform scale, a translation
ANGLE_A, SCALE_A, SHIFT_A = 0.7, (0.9, 1.1, 0.8), (13.0, -21.0, 17.0)
ANGLE_B, SCALE_B, SHIFT_B = -1.3, (1.05, 0.85, 0.95), (-11.0, 19.0, 7.0)


def small_ball():
    return host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1))


def test_abi_names_pose_vertices():
    for name in ("trc_pose_vertices", "trc_download_vertices", "trc_debug_pose_overflows"):
        assert name in abi.DEVICE_SYMBOLS, name
    assert abi.TRC_ABI_VERSION == 13                                  # an addition under 13: the number stays
    assert C.sizeof(abi.Pose) == 144 and abi.Pose.model_matrix.offset == 16 and abi.Pose.normal_matrix.offset == 80
    assert abi.Pose.first.offset == 0 and abi.Pose.count.offset == 4


def other_association(m, v):
    """the same products summed from the right: c0*x + (c1*y + (c2*z + c3))"""
    m = np.asarray(m, dtype=F)
    out = []
    for r in range(3):
        s = m[r, 2] * v[:, 2]
        s = s + m[r, 3]
        t = m[r, 1] * v[:, 1]
        s = t + s
        t = m[r, 0] * v[:, 0]
        out.append(t + s)
    return np.stack(out, axis=1)


def fused(m, v):
    """exact products, summed in float64, rounded once"""
    p = np.concatenate([v[:, :3].astype(np.float64), np.ones((len(v), 1))], axis=1)
    return (p @ np.asarray(m, dtype=np.float64)[:3].T).astype(F)


def test_the_test_matrices_tell_the_definition_from_its_near_misses():
    sc = small_ball()                      # kept alive: its view points into memory the scene owns
    v = rr.vertices_of(sc.view)
    centre = pr.box_centre(v)
    for angle, scale, shift in ((ANGLE_A, SCALE_A, SHIFT_A), (ANGLE_B, SCALE_B, SHIFT_B)):
        model, normal = pr.turn(centre, angle, scale, shift)
        assert F(np.cos(angle)) != np.cos(angle) and F(np.sin(angle)) != np.sin(angle)
        want = pr.pose(v, v, [(0, len(v), model, normal)])
        assert want.dtype == F and (want[:, 6:] == v[:, 6:]).all()
        for near_miss in (other_association, fused):
            assert (near_miss(model, v).view(np.uint32) != want[:, :3].view(np.uint32)).any(), (angle, near_miss.__name__)
        # the normal is the inverse transpose's image, not normalised: a non-uniform scale changes its length
        length = np.linalg.norm(want[:, 3:6].astype(np.float64), axis=1)
        assert (np.abs(length - np.linalg.norm(v[:, 3:6].astype(np.float64), axis=1)) > 1e-3).any()


def test_identity_reproduces_the_rest_values():
    sc = small_ball()                      # kept alive: its view points into memory the scene owns
    v = rr.vertices_of(sc.view)
    v[0, 0] = F(-0.0)
    got = pr.pose(v, v * F(2), [(0, len(v), pr.identity(), pr.identity())])
    assert (got == v).all()                                           # as values ...
    assert not np.signbit(got[0, 0])                                  # ... a -0 comes back as +0


def test_pose_is_from_rest_and_leaves_the_rest_alone():
    sc = small_ball()                      # kept alive: its view points into memory the scene owns
    v = rr.vertices_of(sc.view)
    n = len(v)
    model, normal = pr.turn(pr.box_centre(v), ANGLE_A, SCALE_A, SHIFT_A)
    current = v + F(1)
    got = pr.pose(v, current, [(3, 5, model, normal)])
    assert (got[:3] == current[:3]).all() and (got[8:] == current[8:]).all()
    assert (got[3:8] == pr.pose(v, v, [(0, n, model, normal)])[3:8]).all()


def test_valid_restates_the_refusals():
    i = pr.identity()
    nan = i.copy(); nan[1, 3] = np.nan
    inf_normal = i.copy(); inf_normal[2, 2] = np.inf
    unread = i.copy(); unread[3, :] = np.nan                          # the fourth row is not read
    unread_normal = unread.copy(); unread_normal[:, 3] = np.inf       # nor the normal matrix's fourth column
    assert pr.valid([], 10) and pr.valid([(0, 10, i, i)], 10) and pr.valid([(5, 5, i, i), (0, 5, i, i)], 10)
    assert pr.valid([(0, 10, unread, unread_normal)], 10)
    assert not pr.valid([(0, 0, i, i)], 10)
    assert not pr.valid([(1, 10, i, i)], 10) and not pr.valid([(0xFFFFFFFF, 2, i, i)], 10)
    assert not pr.valid([(0, 5, i, i), (4, 2, i, i)], 10) and not pr.valid([(2, 3, i, i), (2, 3, i, i)], 10)
    assert not pr.valid([(0, 10, nan, i)], 10) and not pr.valid([(0, 10, i, inf_normal)], 10)


def test_refitted_tree_bounds_the_posed_mesh():
    """after a pose the oracle finds through the refitted tree what it finds without any tree"""
    sc = small_ball()
    v0 = rr.vertices_of(sc.view)
    model, normal = pr.turn(pr.box_centre(v0), ANGLE_A, SCALE_A, SHIFT_A)
    v = pr.pose(v0, v0, [(0, len(v0), model, normal)])
    moved = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)
    rays = random_rays(3000, 5, inside_only=True)
    a, b = pyoracle.trace_rays(moved.view, rays), pyoracle.trace_rays(moved.view, rays, brute=True)
    for f in ("hit", "pType", "pIndex", "t"):
        assert (a[f].view(np.uint32) == b[f].view(np.uint32)).all(), f
    assert (a["pType"][a["hit"] != 0] == abi.PRIM_TRIANGLE).any()
