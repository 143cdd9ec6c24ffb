"""trc_skin_bind / trc_skin_vertices on the CPU: the ABI names them without a new version number, the definition (tests/skin_ref.py)
can be told from its near misses on exactly the bindings and palettes the GPU tests use, one-hot influences are a pose, and a tree
refitted around skinned vertices bounds them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_ref as pr
import refit_ref as rr
import skin_ref as sr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_update_vertices import scene
from test_pose_cpu import ANGLE_A, ANGLE_B, SCALE_A, SCALE_B, SHIFT_A, SHIFT_B, small_ball
from tracer_amd import abi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALETTE_SIZES = (3, abi.SKIN_LDS_BONES, abi.SKIN_LDS_BONES + 1, 2048)


def rest_of(residence):
    return rr.vertices_of(scene(residence).view)


def bindings(residence):
    """[(first, count)]: both ends unaligned with a lane, a wavefront and a 256-thread boundary inside the range, and the whole array"""
    n = len(rest_of(residence))
    return [(61, 324), (0, n)] if residence == "mem" else [(3, n - 5), (0, n)]


_PALETTES = {}


def palette_of(residence, n_bones):
    if (residence, n_bones) not in _PALETTES:
        _PALETTES[residence, n_bones] = sr.palette(n_bones, pr.box_centre(rest_of(residence)))
    return _PALETTES[residence, n_bones]


def case(residence, first, count, n_bones):
    """(bones_idx, weights, palette) of one GPU case"""
    return (*sr.binding(count, n_bones), palette_of(residence, n_bones))


CASES = [(r, f, c, nb) for r in ("lds", "mem") for f, c in bindings(r) for nb in PALETTE_SIZES]


def test_abi_names_skin_vertices():
    for name in ("trc_skin_bind", "trc_skin_vertices"):
        assert name in abi.DEVICE_SYMBOLS, name
    assert abi.TRC_ABI_VERSION == 13                                  # an addition under 13: the number stays
    assert C.sizeof(abi.SkinInfluence) == 32 and abi.SkinInfluence.weight.offset == 16
    assert C.sizeof(abi.SkinBone) == 128 and abi.SkinBone.normal_matrix.offset == 64
    assert abi.TRC_SKIN_MAX_BONES == sr.MAX_BONES == 65536
    header = open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
    assert re.search(r"#define\s+TRC_SKIN_MAX_BONES\s+65536u", header)


def test_lds_bound_is_the_csrc_constant():
    text = open(os.path.join(ROOT, "tracer_amd", "csrc", "skin_check.hpp")).read()
    found = re.findall(r"constexpr\s+uint32_t\s+kSkinLdsBones\s*=\s*(\d+)\s*;", text)
    assert len(found) == 1 and int(found[0]) == abi.SKIN_LDS_BONES
    assert 7 * 16 * abi.SKIN_LDS_BONES * 2 <= 160 * 1024            # several workgroups' palettes in a CU's LDS


# ---------------------------------------------------------------------------------------------------- near misses
def transform_then_blend(rest, b, w, palette):
    """every bone poses the vertex, the four results are blended"""
    model, normal = sr.stack(palette)
    out = None
    for k in range(4):
        bm, bn = model[b[:, k], :3, :], normal[b[:, k], :3, :]
        x, y, z = sr.transform(bm, rest[:, 0].copy(), rest[:, 1].copy(), rest[:, 2].copy(), True)
        nx, ny, nz = sr.transform(bn, rest[:, 3].copy(), rest[:, 4].copy(), rest[:, 5].copy(), False)
        p = w[:, k:k + 1] * np.stack([x, y, z, nx, ny, nz], axis=1)
        out = p if out is None else out + p
    return out


def blend_from_the_right(rest, b, w, palette):
    """the blend summed in the order w3 .. w0"""
    return sr.skin(rest, rest, 0, b[:, ::-1], w[:, ::-1], palette)[:, :6]


def blend_in_double(rest, b, w, palette):
    """the blend with exact products, summed in float64 and rounded once"""
    model, normal = sr.stack(palette)
    w64 = w.astype(np.float64)[:, :, None, None]
    bm = (w64 * model.astype(np.float64)[b][:, :, :3, :]).sum(axis=1).astype(F)
    bn = (w64 * normal.astype(np.float64)[b][:, :, :3, :]).sum(axis=1).astype(F)
    x, y, z = sr.transform(bm, rest[:, 0].copy(), rest[:, 1].copy(), rest[:, 2].copy(), True)
    nx, ny, nz = sr.transform(bn, rest[:, 3].copy(), rest[:, 4].copy(), rest[:, 5].copy(), False)
    return np.stack([x, y, z, nx, ny, nz], axis=1)


def normal_from_the_model_matrices(rest, b, w, palette):
    return sr.skin(rest, rest, 0, b, w, [(m, m) for m, _ in palette])[:, :6]


@pytest.mark.parametrize("residence,first,count,n_bones", CASES)
def test_the_test_data_tell_the_definition_from_its_near_misses(residence, first, count, n_bones):
    v0 = rest_of(residence)
    assert len(v0) > 700 if residence == "mem" else len(v0) > 18
    b, w, palette = case(residence, first, count, n_bones)
    assert sr.valid_binding(first, b, w, len(v0)) and sr.valid_palette(palette, b.max())
    assert b.min() == 0 and b.max() == n_bones - 1                   # both ends of the palette are read
    assert (w.sum(axis=1, dtype=np.float64) != 1.0).all() and (w < 0).any() and (w == 0).any()
    assert ((w != 0).all(axis=1)).any() and (b[:, 0] == b[:, 1]).any()
    rest = v0[first:first + count]
    want = sr.skin(v0, v0, first, b, w, palette)[first:first + count]
    assert want.dtype == F and np.array_equal(want[:, 6:].view(np.uint32), rest[:, 6:].view(np.uint32))
    assert (want[:, :6].view(np.uint32) != rest[:, :6].view(np.uint32)).any(axis=1).all()       # every bound vertex moves
    assert np.abs(want[:, :3]).max() < 1e4
    for near_miss in (transform_then_blend, blend_from_the_right, blend_in_double, normal_from_the_model_matrices):
        got = near_miss(rest, b, w, palette)
        assert got.dtype == F and np.allclose(got[:, :3], want[:, :3], rtol=1e-3, atol=1e-2), near_miss.__name__    # near ...
        assert (got.view(np.uint32) != want[:, :6].view(np.uint32)).any(), near_miss.__name__                       # ... and a miss


# ---------------------------------------------------------------------------------------------------- properties
def test_one_hot_influences_are_a_pose():
    sc = small_ball()                      # kept alive: its view points into memory the scene owns
    v = rr.vertices_of(sc.view)
    n = len(v)
    centre = pr.box_centre(v)
    a, b = pr.turn(centre, ANGLE_A, SCALE_A, SHIFT_A), pr.turn(centre, ANGLE_B, SCALE_B, SHIFT_B)
    idx = np.zeros((n, 4), np.int64)
    idx[n // 2:, 0] = 1
    idx[:, 1:] = [1, 0, 1]                                            # any valid bones under the weights of 0
    w = np.zeros((n, 4), F)
    w[:, 0] = 1
    got = sr.skin(v, v, 0, idx, w, [a, b])
    want = pr.pose(v, v, [(0, n // 2, *a), (n // 2, n - n // 2, *b)])
    assert (got == want).all()                                        # as values: a -0 may be a +0


def test_skin_is_from_rest_and_leaves_the_rest_alone():
    sc = small_ball()
    v = rr.vertices_of(sc.view)
    b, w = sr.binding(5, 3)
    palette = sr.palette(3, pr.box_centre(v))
    current = v + F(1)
    got = sr.skin(v, current, 3, b, w, palette)
    assert (got[:3] == current[:3]).all() and (got[8:] == current[8:]).all()
    assert (got[3:8] == sr.skin(v, v, 3, b, w, palette)[3:8]).all()


def test_valid_restates_the_refusals():
    i = pr.identity()
    b, w = sr.binding(6, 4)
    assert sr.valid_binding(4, b, w, 10) and sr.valid_binding(0, b[:0], w[:0], 10) and sr.valid_binding(99, b[:0], w[:0], 10)
    assert not sr.valid_binding(5, b, w, 10) and not sr.valid_binding(0xFFFFFFFF, b, w, 10)
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy(); w2[3, 2] = bad
        assert not sr.valid_binding(0, b, w2, 10)
    b2 = b.copy(); b2[2, 3] = sr.MAX_BONES
    assert not sr.valid_binding(0, b2, w, 10)
    b2[2, 3] = sr.MAX_BONES - 1
    assert sr.valid_binding(0, b2, w, 10)
    nan = i.copy(); nan[1, 3] = np.nan
    inf_normal = i.copy(); inf_normal[2, 2] = np.inf
    unread = i.copy(); unread[3, :] = np.nan                          # the fourth row is not read
    unread_normal = unread.copy(); unread_normal[:, 3] = np.inf       # nor the normal matrix's fourth column
    assert sr.valid_palette([], 3) and sr.valid_palette([(i, i)] * 4, 3) and not sr.valid_palette([(i, i)] * 3, 3)
    assert sr.valid_palette([(i, i), (unread, unread_normal)], 1)
    assert not sr.valid_palette([(i, i), (nan, i)], 0) and not sr.valid_palette([(i, inf_normal), (i, i)], 0)


def test_refitted_tree_bounds_the_skinned_mesh():
    """after a skin the oracle finds through the refitted tree what it finds without any tree"""
    sc = small_ball()
    v0 = rr.vertices_of(sc.view)
    b, w = sr.binding(len(v0), 3)
    v = sr.skin(v0, v0, 0, b, w, sr.palette(3, pr.box_centre(v0)))
    moved = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)
    rays = random_rays(3000, 5, inside_only=True)
    a, c = pyoracle.trace_rays(moved.view, rays), pyoracle.trace_rays(moved.view, rays, brute=True)
    for f in ("hit", "pType", "pIndex", "t"):
        assert (a[f].view(np.uint32) == c[f].view(np.uint32)).all(), f
    assert (a["pType"][a["hit"] != 0] == abi.PRIM_TRIANGLE).any()
