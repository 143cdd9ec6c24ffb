"""What the GPU tests of the kernel census and of the replay matrix take for granted, checked on the CPU: the camera of the replay
matrix (light_oracle_cases.replay_camera) sees what the matrix is about -- rays that escape, an emitter met directly, mesh triangles
of several materials, and on the dense scenes hits the 7-row memo cannot keep -- and the census has a case for every entry of the
kernel tables.  Conditions on the scenes, from the oracle's trace of every camera ray; nothing here is a measurement of the kernels."""
import numpy as np
import pytest

import light_oracle_cases as lc
from tracer_amd import abi

DENSE_W, DENSE_H = 1916, 1076


@pytest.mark.parametrize("scene", sorted(lc.REPLAY_SCENES))
def test_the_replay_camera_sees_what_the_matrix_is_about(scene):
    s = lc.replay_scene(scene)
    dense = scene.startswith("dense")
    W, H = (DENSE_W // 8, DENSE_H // 8) if dense else (lc.W, lc.H)          # the large frame's view at an eighth of its resolution
    cam = lc.replay_camera(*((DENSE_W, DENSE_H) if dense else (W, H)))
    assert cam.lenRadius == 0.0 and all(c != 0.0 for c in (cam.lookFrom.x, cam.lookFrom.y, cam.lookFrom.z))
    h = lc.primary_hits(s, cam, W, H)
    n = W * H
    materials = np.unique(h["material"][h["triangle"]])
    print(f"{scene}: {W} x {H}: escape {1 - h['hit'].mean():.3f}, emitter {h['emitter'].mean():.3f}, triangle pixels {int(h['triangle'].sum())} "
          f"of {len(materials)} materials, uv readers {int(h['uv_read'].sum())}")
    assert (~h["hit"]).sum() >= 0.10 * n
    assert h["emitter"].sum() >= 0.01 * n
    assert h["triangle"].sum() >= 100
    if dense:
        # the dense kernel takes no mesh of more than a dozen triangles (light_oracle_cases.cornell): two of them are in view, one an
        # emitter (the `ends` branch) and one that only a triangle names, or one kept and one that reads uv
        assert len(materials) == 2 and 19 not in materials
        assert (h["emitter"] & h["triangle"]).any() != (h["uv_read"] & h["triangle"]).any()
        assert (h["triangle"] & ~h["emitter"] & ~h["uv_read"]).sum() >= 100
    elif s.tri is not None:
        assert len(materials) >= 5
        assert (h["emitter"] & h["triangle"]).any()                         # an emitter triangle seen directly: the `ends` branch of the twins
    else:
        assert list(materials) == [19]
    if "checker" in scene or "tex" in scene:                                # the cubes are checkered: hits whose colour reads uv
        assert h["uv_read"].sum() >= 100 and (h["uv_read"] & ~h["triangle"]).any()
        assert not lc.kept_pixels(h, 7)[h["uv_read"]].any() and lc.kept_pixels(h, 10).all()
    else:                                                                   # (Cornell's material 6 is a checker: triangles that drew it)
        assert not (h["uv_read"] & ~h["triangle"]).any() and np.all(h["material"][h["uv_read"]] == 6)
    if s.images:
        assert all(s.view.materials[i].textureInfo.type in (abi.TEX_IMAGE, abi.TEX_CHECKER) for i in range(s.view.n_material)
                   if s.view.materials[i].type != abi.MAT_DIFFUSE)


@pytest.mark.parametrize("scene", ["dense-trimat", "dense-trimat-checker"])
def test_the_far_left_camera_sees_the_far_side_of_triangles(scene):
    """hits whose sn is -gn, on a material the 7-row memo keeps and on an emitter"""
    s = lc.replay_scene(scene)
    W, H = DENSE_W // 8, DENSE_H // 8
    h = lc.primary_hits(s, lc.replay_camera(DENSE_W, DENSE_H, 2), W, H)
    assert (h["back"] & ~h["emitter"] & ~h["uv_read"]).sum() >= 20 and (h["back"] & h["emitter"]).any()
    assert h["triangle"][h["back"]].all()
    # ... on a material whose lobe tells sn from -sn (tracePath ends a path on the materials it has no lobe for: they would hide the side)
    kept = np.unique(h["material"][h["back"] & ~h["emitter"] & ~h["uv_read"]])
    assert all(s.view.materials[int(m)].type in (abi.MAT_LAMBERT, abi.MAT_PLASTIC) for m in kept)


def test_the_moved_camera_is_another_eye():
    a, b = lc.replay_camera(lc.W, lc.H), lc.replay_camera(lc.W, lc.H, 1)
    assert all(getattr(a.lookFrom, c) != getattr(b.lookFrom, c) for c in "xyz") and b.lenRadius == 0.0
    ha, hb = (lc.primary_hits(lc.replay_scene("trimat"), c, lc.W, lc.H) for c in (a, b))
    assert (ha["material"] != hb["material"]).mean() > 0.05              # the second launch's memo is not the first's


def test_stacked_views_repeat_the_view():
    s = lc.replay_scene("trimat")
    one = lc.primary_hits(s, lc.replay_camera(lc.W, 46), lc.W, 23)
    two = lc.primary_hits(s, lc.replay_camera(lc.W, 46), lc.W, 46, view_height=23)
    for k in one:
        assert np.array_equal(two[k][:23], one[k]) and np.array_equal(two[k][23:], one[k]), k


def test_the_census_has_a_case_for_every_table_entry():
    """the enumeration by the rule of render_kernels(), and who asserts each entry: the light variants and the plain family's Tex entries
    are tests/test_gpu_light_oracle.py's, the two dense entries have a test of their own, every other one a census case"""
    entries = lc.table_entries()
    assert len(entries) == len(set(entries)) == 134
    assert {e[2] for e in entries} == set(abi.KERNEL_VARIANTS) and {e[4] for e in entries} == set(abi.KERNEL_SHAPES)
    cases = lc.census_cases()
    claimed = {c.entry for c in cases}
    assert len(claimed) == len(cases) == 77 and len({c.id for c in cases}) == 77
    elsewhere = {e for e in entries if e[2] in lc.LIGHT_VARIANTS or (e[0] == "plain" and e[2] == "tex") or e[4] == "dense"}
    assert claimed | elsewhere == set(entries) and not (claimed & elsewhere)
    assert sum(e[4] == "dense" for e in entries) == 2
    for c in cases:
        family, integ, variant, residence, shape = c.entry
        assert (c.scene.tri is not None) == (family == "trimat") and bool(c.scene.images) == (variant == "tex")
        assert c.spp == (2 if shape == "strip" else 8) and c.env_rgb != (0.0, 0.0, 0.0)
    # a variant or a shape the census has not heard of is taken to be in every table: it shows as unreached
    assert lc._in_table(lc.PATH, "brand_new", "lds", "one") and lc._in_table(lc.VOLUME, "plain", "lds", "brand_new")
