"""The geometry side of libtracer_amd_fast.so (the same sources under -ffp-contract=fast, approximate division / sqrt, flushed denormals)
through the public C ABI: device-built trees, the refit family, recomputed normals, moved primitives, hidden triangles, rebuilds, the
tree cost, and camera rays through all of those trees.  What min / max and exact products make bit-exact in any flavour is asserted bit
for bit against the definitions (tests/refit_ref.py) and the exact build; what rounds is held to the float64 restatements and running
bounds of tests/fast_ref.py, and to no other tolerance.  Structure comes first: a builder whose count and partition kernels disagreed on
a leaf's bucket would mis-size a child range, and validate_tree would say so.  The exact build (`gpu`) is the reference; the code under
test is the fast library (`fast`) alone.  Measured tree-quality ratios: profiles/r29/fast_flavour.txt."""
import ctypes as C

import numpy as np
import pytest

import fast_ref as fr
import morph_ref as mr
import pose_ref as pr
import primitives_ref as pm
import rebuild_ref as rb
import refit_ref as rr
import skin_ref as sr
import visibility_ref as vr
from test_fast_ref_cpu import (BONES, RAY_H, RAY_W, TWIST, fused_case, hidden_mask, indices_of, ray_view, rest_of, robust, view_rays)
from test_gpu_morph_vertices import small_case as morph_case
from test_gpu_pose_vertices import bits, matrices, table
from test_gpu_sah_device import leaf_records
from test_gpu_skin_vertices import small_case as skin_case
from test_gpu_update_vertices import DEVICE_TREE, first_difference, scene
from tracer_amd import abi, device, host

pytestmark = pytest.mark.gpu
F = np.float32
SAH, SAH3 = abi.TREE_SAH, abi.TREE_SAH | abi.TREE_SAH3
BUILDERS = ("sah", "device_sah", "device_sah3", "lbvh")
LEAF_COUNTS = (2, 3, 64, 65, 257)             # either side of the builder's small-subtree (64) and wide-node paths
# interior_half_area of the fast build's tree over that of the exact build's from the same leaves.  The largest excess measured over every
# builder and leaf set of this file is 0 (profiles/r29/fast_flavour.txt), so 1 + twice that excess is 1.  Mind what that means: three trees
# ("mem" under the SAH builds) already differ from the exact build's record for record without costing more, and any later change -- a
# compiler that rounds a split cost the other way -- that makes one of them dearer by a single ulp fails this test.  That is a finding to
# explain and then to measure again by the same rule (never above 1.10), not a bound to pad in advance.
QUALITY_BOUND = 1.0


@pytest.fixture(scope="module")
def fast():
    t = device.Tracer(0, fast_math=True)
    yield t
    t.close()


def analytic(residence):
    return scene(residence, analytic_leaves_only=True)


def build(t, builder, leaves_view, analytic_view):
    """one of the four device builds; the leaf-list cases pass one view for both (they have no triangles)"""
    if builder == "sah":
        t.upload_scene_sah(leaves_view)
    elif builder == "lbvh":
        t.upload_scene_lbvh(leaves_view)
    else:
        t.upload_scene_device(analytic_view, (SAH if builder == "device_sah" else SAH3) | abi.TREE_TRIANGLE_LEAVES)


_LISTS = {}


def leaf_list_view(n):
    """n random sphere leaves (tests/test_gpu_sah_device.py's records) as a leaves view; free of denormals"""
    if n not in _LISTS:
        sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
        rng = np.random.default_rng(100 + n)
        c = rng.uniform(-50, 50, (n, 3)).astype(F); r = rng.uniform(0.01, 3.0, (n, 3)).astype(F)
        assert fr.free_of_denormals(c - r, c + r)
        leaves = leaf_records(list(zip(c - r, c + r)), sc.view.n_sphere)
        v = abi.Scene.from_buffer_copy(sc.leaves_view()); v.bvhList = C.cast(leaves, C.POINTER(abi.BVH)); v.n_bvh = n
        _LISTS[n] = (sc, leaves, v)
    return _LISTS[n][2]


def views_of(case):
    if isinstance(case, int):
        return leaf_list_view(case), leaf_list_view(case)
    return scene(case).leaves_view(), analytic(case).view


def sorted_leaves(records):
    """the leaf records' (pType, pIndex, box words), sorted: what a builder may not change"""
    a = fr.raw(records)
    leaf = a[a[:, fr.PTYPE] != fr.PRIM_BVH][:, [4, 5, 8, 9, 10, 12, 13, 14]]
    return leaf[np.lexsort(leaf.T[::-1])]


def check_valid(records, expected, info=None):
    message, depth = fr.validate_tree(records, expected)
    assert message == "", message
    if info is not None:
        assert info[0] == len(fr.raw(records)) and info[1] == depth, (info, depth)
    return depth


# --------------------------------------------------------------------------------------------------- builders
@pytest.mark.parametrize("case", LEAF_COUNTS + ("lds", "mem"), ids=str)
@pytest.mark.parametrize("builder", BUILDERS)
def test_device_built_tree_is_a_tree_over_the_exact_build_s_leaves(gpu, fast, builder, case):
    leaves_view, analytic_view = views_of(case)
    build(gpu, builder, leaves_view, analytic_view)
    want = fr.raw(gpu.download_bvh())
    exact_cost = gpu.tree_cost()
    build(fast, builder, leaves_view, analytic_view)
    got = fr.raw(fast.download_bvh())
    check_valid(got, fr.leaves_of(want), fast.lbvh_info())
    assert np.array_equal(sorted_leaves(got), sorted_leaves(want))            # leaf boxes: the exact build's bits
    cost = fast.tree_cost()
    assert (cost.n_interior, cost.n_leaves) == (exact_cost.n_interior, exact_cost.n_leaves)
    if exact_cost.interior_half_area > 0:
        ratio = cost.interior_half_area / exact_cost.interior_half_area
        print(f"quality {builder} {case}: interior_half_area fast / exact = {ratio:.17g}, records equal: {np.array_equal(got, want)}")
        assert ratio <= QUALITY_BOUND
    else:
        assert cost.interior_half_area == 0                                    # two leaves: no interior child slot


# --------------------------------------------------------------------------------------------------- refit
@pytest.mark.parametrize("single", [0, 1], ids=["per_depth", "single_launch"])
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_refit_is_the_definition_s_bit_for_bit(residence, builder, single):
    with device.Tracer(0, fast_math=True) as t:
        t.debug_set("refit_single", single)
        build(t, builder, *views_of(residence))
        before = rr.raw(t.download_bvh())
        idx = indices_of(residence)
        for angle in (0.5, -1.2):
            v = rr.twist(rest_of(residence), angle)
            assert fr.free_of_denormals(v)
            t.update_vertices(v)
            got = rr.raw(t.download_bvh())
            assert not first_difference(got, rr.refit(before, v, idx)), angle          # min and max are exact
        assert np.array_equal(bits(t.download_vertices()), bits(v))


# --------------------------------------------------------------------------------------------------- pose, skin, morph, fused
def tree_follows(t, before, residence):
    """the tree after an animation call is refit_ref.refit of the tree before with the DOWNLOADED vertices, bit for bit"""
    got = rr.raw(t.download_bvh())
    assert not first_difference(got, rr.refit(before, t.download_vertices(), indices_of(residence)))
    assert t.pose_overflows() == 0


def assert_within(got, t, rows=None):
    ok = fr.within(got, t)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, f"{len(bad)} components outside the bound, first {bad[0]}: got {got[tuple(bad[0])]!r}, value {t.v[tuple(bad[0])]!r}, bound {fr.bound(t)[tuple(bad[0])]!r}"
    assert np.array_equal(bits(got[:, 6:]), bits(t.v[:, 6:].astype(F)))                        # uv: copied bit for bit
    if rows is not None:                                                                         # untouched vertices: bound 0, so bits
        assert not fr.bound(t)[~rows].any()


def start(t, residence):
    t.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    return rest_of(residence), rr.raw(t.download_bvh())


@pytest.mark.parametrize("name", ["ragged", "whole"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_posed_vertices_within_the_bound(fast, residence, name):
    v0, before = start(fast, residence)
    poses = table(residence, name)
    assert fr.free_of_denormals(v0, *[m for p in poses for m in p[2:]])
    fast.pose_vertices(poses)
    got = fast.download_vertices()
    assert_within(got, fr.pose(v0, v0, poses))
    tree_follows(fast, before, residence)
    ident = [(0, len(v0), pr.identity(), pr.identity())]
    fast.pose_vertices(ident)                                                                    # an identity pose: the rest values
    assert np.array_equal(fast.download_vertices(), v0)
    tree_follows(fast, before, residence)


@pytest.mark.parametrize("n_bones,no_lds", [(3, 0), (3, 1), (abi.SKIN_LDS_BONES + 1, 0)])
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_skinned_vertices_within_the_bound(fast, residence, which, n_bones, no_lds):
    v0, before = start(fast, residence)
    first, b, w, palette = skin_case(residence, which, n_bones)
    assert fr.free_of_denormals(v0, w, *sr.stack(palette)) and (w < 0).any()
    fast.debug_set("skin_no_lds", no_lds)
    try:
        fast.skin_bind(b, w, first=first)
        fast.skin_vertices(palette)
        got = fast.download_vertices()
    finally:
        fast.debug_set("skin_no_lds", 0)
    assert_within(got, fr.skin(v0, v0, first, b, w, palette))
    tree_follows(fast, before, residence)


@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_morphed_vertices_within_the_bound(fast, residence, which, n_targets):
    v0, before = start(fast, residence)
    first, d, w = morph_case(residence, which, n_targets, "negative")
    assert fr.free_of_denormals(v0, d, w) and (w < 0).any()
    fast.morph_bind(d, first=first)
    fast.morph_vertices(w)
    got = fast.download_vertices()
    assert_within(got, fr.morph(v0, v0, first, d, w))
    assert (bits(got[first:first + d.shape[1]]) != bits(v0[first:first + d.shape[1]])).any(axis=1).all()
    tree_follows(fast, before, residence)
    fast.morph_vertices(mr.weights(n_targets, "zero"))                                          # zero weights: the rest bits exactly
    assert np.array_equal(bits(fast.download_vertices()), bits(v0))
    tree_follows(fast, before, residence)


@pytest.mark.parametrize("n_bones", BONES)
@pytest.mark.parametrize("layout", ["identical", "overlap", "apart"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_fused_vertices_and_recomputed_normals_within_the_bound(fast, residence, layout, n_bones):
    v0, before = start(fast, residence)
    mf, d, w, sf, b, sw, palette = fused_case(residence, layout, n_bones)
    fast.morph_bind(d, first=mf)
    fast.skin_bind(b, sw, first=sf)
    fast.morph_vertices(w, palette)
    got = fast.download_vertices()
    assert_within(got, fr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette))
    tree_follows(fast, before, residence)
    # trc_recompute_normals of what the device now holds (its inputs are `got`, binary32 values like any other)
    tree = rr.raw(fast.download_bvh())
    idx = indices_of(residence)
    first, count = 3, len(v0) - 7
    fast.recompute_normals(first, count)
    after = fast.download_vertices()
    new, length, decided = fr.normals(got, idx, first, count)
    assert decided.sum() > 0.9 * count
    assert fr.within(after[:, 3:6], new)[decided].all()
    got_length = np.sqrt((after[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(got_length - 1.0) <= fr.bound(length))[decided].all()
    import normals_ref as nr
    alone = ~nr.in_range(len(v0), first, count)
    alone[nr.kept(got, idx)] = True
    assert np.array_equal(bits(after[alone]), bits(got[alone]))                                 # vertices the definition leaves alone
    assert np.array_equal(bits(after[:, :3]), bits(got[:, :3])) and np.array_equal(bits(after[:, 6:]), bits(got[:, 6:]))
    assert not first_difference(rr.raw(fast.download_bvh()), tree)                              # positions and every box unchanged


# --------------------------------------------------------------------------------------------------- update_primitives
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_moved_primitives_leaf_boxes_within_the_bound(fast, residence):
    sc = scene(residence)
    fast.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    before = rr.raw(fast.download_bvh())
    sp, sq, cb = pm.motion(sc.view)                                                              # a sphere, the light square and a cube move
    fast.update_primitives(spheres=sp, squares=sq, cubes=cb)
    got = rr.raw(fast.download_bvh())
    assert (got[:, :8] == before[:, :8]).all()
    box = got.view(F)
    lists = {abi.PRIM_SPHERE: sp, abi.PRIM_SQUARE: sq, abi.PRIM_CUBE: cb}
    n_checked = 0
    for i in range(len(got)):
        t = int(got[i, fr.PTYPE])
        if t in lists:
            rec = lists[t][int(got[i, fr.PINDEX])]
            lo, hi = fr.primitive_leaf_box(*pm._box3(rec.box if t == abi.PRIM_CUBE else rec.boundingBOX), pm._cols(rec.model_matrix))
            assert fr.within(box[i, fr.MINI], lo).all() and fr.within(box[i, fr.MAXI], hi).all(), (i, t)
            n_checked += 1
    assert n_checked >= len(sq) + 1 and (got[:, 8:] != before[:, 8:]).any()
    # interior boxes: the union of their children, bit for bit; triangle leaves keep their boxes
    assert not first_difference(got, rr.refit(got, rest_of(residence), indices_of(residence)))
    assert fr.validate_tree(got, fr.leaves_of(before))[0] == ""
    # the square record's 1 / (2 di dj): a hit on the moved light square reports it as its PDF
    rays = view_rays()
    hits = fast.trace_rays(rays, production=True)
    on = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_SQUARE)
    seen = 0
    for k in np.unique(hits["pIndex"][on]):
        t = fr.square_pdf((sq[k].range_i.x, sq[k].range_i.y), (sq[k].range_j.x, sq[k].range_j.y))
        assert fr.within(hits["PDF"][on & (hits["pIndex"] == k)], t).all(), k
        seen += 1
    assert seen >= 3


# --------------------------------------------------------------------------------------------------- visibility and rebuild
@pytest.mark.parametrize("flags", [0, SAH, SAH3], ids=["lbvh", "sah", "sah3"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_hidden_triangles_and_rebuilds_after_a_pose(fast, residence, flags):
    v0, before = start(fast, residence)
    idx = indices_of(residence)
    n_tri = len(idx) // 3
    fast.pose_vertices(table(residence, "whole"))
    posed = fast.download_vertices()
    analytic_leaves = [l for l in fr.leaves_of(before) if l[0] != abi.PRIM_TRIANGLE]
    mask = hidden_mask(residence)
    ranges = vr.ranges_of(np.ones(n_tri, np.uint8), mask)
    fast.set_triangle_visibility(ranges, flags)
    assert np.array_equal(fast.triangle_visibility(), mask)                                      # the host's model of the mask
    tree = rr.raw(fast.download_bvh())
    visible = [(abi.PRIM_TRIANGLE, int(t)) for t in np.nonzero(mask)[0]]
    check_valid(tree, analytic_leaves + visible, fast.lbvh_info())
    # triangles move while hidden (a pose by other matrices), then come back: with the boxes of their current vertices
    fast.pose_vertices(table(residence, "whole", "B"))
    moved = fast.download_vertices()
    assert (bits(moved) != bits(posed)).any()
    fast.set_triangle_visibility([(0, n_tri, 1)], flags)
    assert fast.triangle_visibility().all()
    tree = rr.raw(fast.download_bvh())
    check_valid(tree, analytic_leaves + [(abi.PRIM_TRIANGLE, t) for t in range(n_tri)], fast.lbvh_info())
    assert not first_difference(tree, rr.refit(tree, moved, idx))                                # every triangle leaf: its current vertices' box
    # a rebuild keeps every leaf box's bits
    for again in (SAH, 0, SAH3):
        fast.rebuild_tree(again)
        rebuilt = rr.raw(fast.download_bvh())
        check_valid(rebuilt, fr.leaves_of(tree), fast.lbvh_info())
        assert np.array_equal(sorted_leaves(rebuilt), sorted_leaves(tree)), again
    assert np.array_equal(bits(fast.download_vertices()), bits(moved))


# --------------------------------------------------------------------------------------------------- tree cost
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_tree_cost_of_a_caller_s_tree_agrees_with_the_exact_build_s(gpu, fast, residence):
    """the same caller's tree in both flavours: equal counts, and each flavour's three sums within the header's (n - 1) 2^-53 of the
    definition summed on the host (rebuild_ref.tree_cost: math.fsum over the binary64 terms)"""
    view = ray_view(residence, "moved")                                                          # a caller's tree, refitted on the host
    gpu.upload_scene(view); fast.upload_scene(view)
    a, b = gpu.tree_cost(), fast.tree_cost()
    tree = np.frombuffer(C.string_at(view.bvhList, 64 * view.n_bvh), dtype=np.uint32).reshape(-1, 16)
    ref = rb.tree_cost(tree)
    want = dict(root_half_area=ref["root"], interior_half_area=ref["interior"], leaf_half_area=ref["leaf"])
    assert (a.n_interior, a.n_leaves) == (b.n_interior, b.n_leaves) and a.n_leaves > 2
    n = a.n_leaves
    for name in ("root_half_area", "interior_half_area", "leaf_half_area"):
        exact = want[name]                                                                       # math.fsum of the definition's terms
        for flavour, x in (("exact", getattr(a, name)), ("fast", getattr(b, name))):
            assert exact > 0 and abs(x - exact) <= (n - 1) * 2.0 ** -53 * exact, (name, flavour)  # the header's (n - 1) 2^-53


# --------------------------------------------------------------------------------------------------- rays
T_RELATIVE = 1e-3                                # tests/test_gpu_fast_math.py's stated tolerance on t


def check_rays(gpu, fast, residence, kind, label):
    rays = view_rays()
    gpu.upload_scene(ray_view(residence, kind))                                                  # the host tree of the same geometry
    want, got = gpu.trace_rays(rays, production=True), fast.trace_rays(rays, production=True)
    ok = robust(residence, kind)
    assert 1.0 - ok.mean() <= fr.MAX_NON_ROBUST
    for f in ("hit", "pType", "pIndex"):
        bad = np.nonzero(ok & (got[f] != want[f]))[0]
        assert len(bad) == 0, f"{label}: {f} of {len(bad)} robust rays differs, first ray {bad[0]}"
    h = ok & (want["hit"] != 0)
    assert h.sum() > 0.5 * len(rays)
    assert (np.abs(got["t"][h].astype(np.float64) - want["t"][h]) <= T_RELATIVE * want["t"][h]).all(), label


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_robust_rays_hit_what_the_exact_build_hits(gpu, fast, residence):
    assert len(view_rays()) == RAY_W * RAY_H
    fast.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    check_rays(gpu, fast, residence, "uploaded", "uploaded")
    fast.update_vertices(rr.twist(rest_of(residence), TWIST))
    check_rays(gpu, fast, residence, "moved", "refitted")
    for flags in (SAH, 0, SAH3):
        fast.rebuild_tree(flags)
        check_rays(gpu, fast, residence, "moved", f"rebuilt {flags}")
    mask = hidden_mask(residence)
    fast.set_triangle_visibility(vr.ranges_of(np.ones(len(mask), np.uint8), mask), SAH)
    check_rays(gpu, fast, residence, "hidden", "hidden")


# --------------------------------------------------------------------------------------------------- determinism
def sequence(t, residence):
    """build, pose, fused morph + skin, normals, hide, rebuild, a 32 x 32 frame -> everything downloadable, as bytes"""
    out = []
    v0 = rest_of(residence)
    t.upload_scene_device(analytic(residence).view, SAH3 | abi.TREE_TRIANGLE_LEAVES)
    out.append(rr.raw(t.download_bvh()).tobytes())
    t.pose_vertices(table(residence, "ragged"))
    out.append(t.download_vertices().tobytes()); out.append(rr.raw(t.download_bvh()).tobytes())
    mf, d, w, sf, b, sw, palette = fused_case(residence, "overlap", 3)
    t.morph_bind(d, first=mf); t.skin_bind(b, sw, first=sf)
    t.morph_vertices(w, palette)
    t.recompute_normals()
    out.append(t.download_vertices().tobytes()); out.append(rr.raw(t.download_bvh()).tobytes())
    mask = hidden_mask(residence)
    t.set_triangle_visibility(vr.ranges_of(np.ones(len(mask), np.uint8), mask), SAH)
    out.append(rr.raw(t.download_bvh()).tobytes())
    t.rebuild_tree(0)
    out.append(rr.raw(t.download_bvh()).tobytes())
    t.set_camera(host.prepare_camera(32, 32)); t.set_environment((0.0, 0.0, 0.0)); t.resize(32, 32)
    t.seed(5); t.clear_accum(); t.render(spp=4, integrator=abi.INTEGRATOR_MIS)
    out.append(t.download_accum().tobytes()); out.append(t.download_rng().tobytes())
    return out


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_a_second_fast_context_gives_the_same_bits(fast, residence):
    first = sequence(fast, residence)
    with device.Tracer(0, fast_math=True) as other:
        second = sequence(other, residence)
    assert [a == b for a, b in zip(first, second)] == [True] * len(first)
    assert np.frombuffer(first[-2], F).any()
