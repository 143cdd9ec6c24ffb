"""tests/fast_ref.py on the CPU: what the fast-math build is held to must itself hold.  The exact binary32 definitions (pose_ref,
skin_ref, morph_ref, normals_ref, primitives_ref, adaptive_ref) lie within every bound of their float64 restatement on the cases the GPU
tests use, so the reference alone passes; a deliberately wrong variant lies outside it; the tree validator rejects doctored trees; at
most 10 % of the camera rays of every view the GPU tests trace are non-robust.  The case builders here are the GPU modules' too."""
import numpy as np
import pytest

import adaptive_ref as ar
import fast_ref as fr
import morph_ref as mr
import normals_ref as nr
import pose_ref as pr
import primitives_ref as pm
import rebuild_ref as rb
import refit_ref as rr
import skin_ref as sr
import visibility_ref as vr
from conftest import camera_rays
from test_gpu_adaptive import uploaded_planes
from test_gpu_morph_vertices import layouts
from test_gpu_morph_vertices import small_case as morph_case
from test_gpu_pose_vertices import matrices, table
from test_gpu_skin_vertices import small_case as skin_case
from test_gpu_update_vertices import scene
from test_morph_cpu import deltas_of
from test_skin_cpu import palette_of
from tracer_amd import abi, host

F = np.float32
RESIDENCES = ("lds", "mem")
BONES = (3, abi.SKIN_LDS_BONES + 1)
RAY_W, RAY_H = 160, 90
TWIST = 0.7                                  # refit_ref.twist's angle for the refitted, rebuilt and hidden views
VIEW_KINDS = ("uploaded", "moved", "hidden")


def rest_of(residence):
    return rr.vertices_of(scene(residence).view)


def indices_of(residence):
    return rr.indices_of(scene(residence).view)


def fused_case(residence, layout, n_bones):
    """(morph first, deltas, weights, skin first, bones, skin weights, palette) of tests/test_gpu_morph_vertices.py's fused test"""
    n = len(rest_of(residence))
    (mf, mc), (sf, sc_) = layouts(n)[layout]
    b, sw = sr.binding(sc_, n_bones)
    return mf, deltas_of(mc, 3), mr.weights(3, "negative"), sf, b, sw, palette_of(residence, n_bones)


def hidden_mask(residence):
    """the middle half of the index list hidden"""
    n = scene(residence).view.n_index // 3
    m = np.ones(n, np.uint8)
    m[n // 4:n // 4 + n // 2] = 0
    return m


_VIEWS, _ROBUST = {}, {}


def ray_view(residence, kind):
    """a scene view (kept alive in the cache) over a HOST-built tree of the geometry a GPU test traces: the upload's; the mesh twisted
    by TWIST (the refitted and the rebuilt tree bound the same triangles); the twisted mesh with hidden_mask's triangles left out"""
    key = (residence, kind)
    if key not in _VIEWS:
        sc = scene(residence)
        if kind == "uploaded":
            _VIEWS[key] = rr.Moved(sc.view, sc.bvh_array().copy(), rest_of(residence))
        else:
            v = rr.twist(rest_of(residence), TWIST)
            tree = rr.refit(sc.bvh_array().copy(), v, indices_of(residence))
            if kind == "hidden":
                tree = rb.expected_tree(vr.leaf_list(tree, False, v, indices_of(residence), hidden_mask(residence)), True)
            _VIEWS[key] = rr.Moved(sc.view, tree, v)
    return _VIEWS[key].view


def view_rays():
    return camera_rays(host.prepare_camera(RAY_W, RAY_H), RAY_W, RAY_H)


def robust(residence, kind):
    key = (residence, kind)
    if key not in _ROBUST:
        _ROBUST[key] = fr.robust_rays(ray_view(residence, kind), view_rays())
    return _ROBUST[key]


def inside(got, t):
    return bool(fr.within(got, t).all())


# ---------------------------------------------------------------------------------------------------- the reference alone passes
@pytest.mark.parametrize("residence", RESIDENCES)
def test_inputs_are_free_of_denormals(residence):
    v0 = rest_of(residence)
    assert fr.free_of_denormals(v0, *matrices(residence, "A"), *matrices(residence, "B"), deltas_of(len(v0), 3))
    for nb in BONES:
        assert fr.free_of_denormals(*sr.stack(palette_of(residence, nb)))
    assert not fr.free_of_denormals(np.array([1e-40], F)) and fr.free_of_denormals(np.array([0.0, -0.0, 2.0 ** -126], F))


@pytest.mark.parametrize("name", ["ragged", "whole"])
@pytest.mark.parametrize("residence", RESIDENCES)
def test_pose_definition_within_the_bound(residence, name):
    v0, poses = rest_of(residence), table(residence, name)
    t = fr.pose(v0, v0, poses)
    assert inside(pr.pose(v0, v0, poses), t) and fr.bound(t).max() > 0
    assert (fr.bound(t)[:, 6:] == 0).all()                                                    # uv: copied
    ident = [(0, len(v0), pr.identity(), pr.identity())]
    assert np.array_equal(fr.pose(v0, v0, ident).v, v0.astype(np.float64))                     # an identity pose: the rest values


@pytest.mark.parametrize("n_bones", BONES)
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", RESIDENCES)
def test_skin_definition_within_the_bound_and_a_wrong_blend_outside(residence, which, n_bones):
    v0 = rest_of(residence)
    first, b, w, palette = skin_case(residence, which, n_bones)
    t = fr.skin(v0, v0, first, b, w, palette)
    assert inside(sr.skin(v0, v0, first, b, w, palette), t)
    # the influences blended in another order (inside: a reordered sum differs by roundings only) ...
    reordered = fr.skin(v0, v0, first, b, w, palette, order=(3, 2, 1, 0))
    assert inside(reordered.v.astype(F), t)
    # ... and in another order with one dropped (outside)
    dropped = fr.skin(v0, v0, first, b, w, palette, order=(3, 1, 0))
    rows = slice(first, first + len(b))
    assert not fr.within(dropped.v.astype(F), t)[rows, :3].all(axis=1).any() or (w[:, 2] == 0).any()
    lost = w[:, 2] != 0
    assert lost.any() and not fr.within(dropped.v.astype(F), t)[rows, :3][lost].all(axis=1).any()


@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", RESIDENCES)
def test_morph_definition_within_the_bound_and_a_skipped_target_outside(residence, which, n_targets):
    v0 = rest_of(residence)
    first, d, w = morph_case(residence, which, n_targets, "negative")
    assert (w < 0).any()
    t = fr.morph(v0, v0, first, d, w)
    assert inside(mr.morph(v0, v0, first, d, w), t)
    skipped = fr.morph(v0, v0, first, d, w, skip=(0,))
    rows = slice(first, first + d.shape[1])
    assert not fr.within(skipped.v.astype(F), t)[rows, :3].all(axis=1).any()
    zero = fr.morph(v0, v0, first, d, mr.weights(n_targets, "zero"))
    assert np.array_equal(zero.v, v0.astype(np.float64)) and not zero.e.any()                  # zero weights: the rest, bound 0


@pytest.mark.parametrize("n_bones", BONES)
@pytest.mark.parametrize("layout", ["identical", "overlap", "apart"])
@pytest.mark.parametrize("residence", RESIDENCES)
def test_fused_definition_within_the_bound(residence, layout, n_bones):
    v0 = rest_of(residence)
    mf, d, w, sf, b, sw, palette = fused_case(residence, layout, n_bones)
    t = fr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette)
    assert inside(mr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette), t)


@pytest.mark.parametrize("residence", RESIDENCES)
def test_normals_definition_within_the_bound_and_unnormalised_outside(residence):
    v0, idx = rest_of(residence), indices_of(residence)
    mf, d, w, sf, b, sw, palette = fused_case(residence, "overlap", 3)
    v = mr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette)
    want = nr.recompute(v, idx)
    new, length, decided = fr.normals(v, idx)
    assert decided.sum() > 0.9 * len(v)
    assert fr.within(want[:, 3:6], new)[decided].all()
    got_length = np.sqrt((want[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(got_length - 1.0) <= fr.bound(length))[decided].all()
    raw, raw_length, _ = fr.normals(v, idx, normalise=False)
    assert not (np.abs(raw_length.v - 1.0) <= fr.bound(length))[decided].any()                # a normal left unnormalised


@pytest.mark.parametrize("residence", RESIDENCES)
def test_primitive_boxes_and_the_square_record_within_the_bound(residence):
    sp, sq, cb = pm.motion(scene(residence).view)
    for ptype, recs in ((abi.PRIM_SPHERE, sp), (abi.PRIM_SQUARE, sq), (abi.PRIM_CUBE, cb)):
        for rec in recs:
            box = rec.box if ptype == abi.PRIM_CUBE else rec.boundingBOX
            cols = pm._cols(rec.model_matrix)
            assert fr.free_of_denormals(np.array(cols, F))
            lo, hi = fr.primitive_leaf_box(*pm._box3(box), cols)
            want = pm.primitive_leaf_box(ptype, rec)
            assert inside(want[0], lo) and inside(want[1], hi)
    for s in sq:
        t = fr.square_pdf((s.range_i.x, s.range_i.y), (s.range_j.x, s.range_j.y))
        pdf = pm.pack_square(s)[5:6].view(F)[0]
        assert inside(pdf, t) and not inside(np.nextafter(pdf, F(1), dtype=F) * F(1 + 2.0 ** -18), t)


def test_tile_error_definition_within_the_bound():
    I, A = uploaded_planes()
    t = fr.tile_errors(I, A)
    want = ar.tile_errors(I, A)
    assert np.isfinite(t.v).all() and np.isfinite(t.e).all()
    assert inside(want, t), (want, t.v, fr.bound(t))
    assert not inside(ar.tile_errors(I * F(1.01), A), t)                                        # another frame is outside


# ---------------------------------------------------------------------------------------------------- the validator
def a_tree():
    sc = scene("lds")
    tree = sc.bvh_array().copy()
    return tree, fr.leaves_of(tree)


def test_validator_accepts_the_host_trees():
    for residence in RESIDENCES:
        tree = scene(residence).bvh_array().copy()
        message, depth = fr.validate_tree(tree, fr.leaves_of(tree))
        assert message == "" and depth == scene(residence).tree_depth()
        v = rr.twist(rest_of(residence), TWIST)
        assert fr.validate_tree(rr.refit(tree, v, indices_of(residence)), fr.leaves_of(tree))[0] == ""


def ulp(x, up):
    return np.nextafter(x, F(np.inf) if up else F(-np.inf))


def test_validator_rejects_doctored_trees():
    tree, leaves = a_tree()
    interior = np.nonzero(tree[:, fr.PTYPE] == fr.PRIM_BVH)[0]
    leaf = np.nonzero(tree[:, fr.PTYPE] != fr.PRIM_BVH)[0]
    # a leaf twice (and so another missing)
    t = tree.copy(); t[leaf[3], [fr.PTYPE, fr.PINDEX]] = t[leaf[4], [fr.PTYPE, fr.PINDEX]]
    assert "twice" in fr.validate_tree(t, leaves)[0]
    # a leaf missing: the expected list names one the tree does not hold
    assert "missing" in fr.validate_tree(tree, leaves[:-1] + [(abi.PRIM_TRIANGLE, 10 ** 6)])[0]
    assert "records for" in fr.validate_tree(tree, leaves[:-1])[0]
    # a child box grown or shrunk by one ulp: its parent is no longer the union
    child = int(tree[interior[2], fr.LEFT])
    for up in (True, False):
        for col in (8, 13):
            t = tree.copy(); b = t.view(F); b[child, col] = ulp(b[child, col], up)
            message = fr.validate_tree(t, leaves)[0]
            assert "union" in message, (up, col, message)
    # a dangling child, a child with two parents, a wrong parent link, a second root
    t = tree.copy(); t[interior[1], fr.RIGHT] = len(tree) + 5
    assert "dangling" in fr.validate_tree(t, leaves)[0]
    t = tree.copy(); t[interior[1], fr.RIGHT] = t[interior[2], fr.LEFT]
    assert fr.validate_tree(t, leaves)[0]
    t = tree.copy(); t[child, fr.PARENT] = interior[5]
    assert "parent" in fr.validate_tree(t, leaves)[0]
    t = tree.copy(); t[0, fr.PARENT] = 3
    assert "root" in fr.validate_tree(t, leaves)[0]
    assert "depth" in fr.validate_tree(tree, leaves, max_depth=2)[0]
    assert fr.validate_tree(tree, leaves)[0] == ""


# ---------------------------------------------------------------------------------------------------- robust rays
@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("residence", RESIDENCES)
def test_at_most_a_tenth_of_a_view_s_rays_is_not_robust(residence, kind):
    ok = robust(residence, kind)
    print(residence, kind, "non-robust", 1.0 - ok.mean())
    assert len(ok) == RAY_W * RAY_H and 1.0 - ok.mean() <= fr.MAX_NON_ROBUST
    assert not ok.all()                                                                          # the filter does filter: silhouettes
    from oracle import pyoracle
    hits = pyoracle.trace_rays(ray_view(residence, kind), view_rays())
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert (tri & ok).sum() > 50                                                                 # ... and the mesh is in the picture
    if kind == "hidden":
        assert hidden_mask(residence)[hits["pIndex"][tri]].all()
