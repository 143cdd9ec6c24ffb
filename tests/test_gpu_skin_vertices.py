"""trc_skin_bind / trc_skin_vertices on the GPU (include/tracer_abi.h): the skinned vertices against the definition
(tests/skin_ref.py) bit for bit, for both palette paths of the kernel (staged in LDS, gathered from memory), and everything behind them
-- tree, frames, what is kept and what is dropped -- against what trc_update_vertices leaves for the same vertices, against the
definition of the refit (tests/refit_ref.py), against a pose where the influences are one-hot, and against the CPU oracle.  The bindings
(tests/test_skin_cpu.py) put a lane, a wavefront and a 256-thread boundary inside the bound range, with both of its ends unaligned."""
import os
import subprocess

import numpy as np
import pytest

import pose_ref as pr
import refit_ref as rr
import skin_ref as sr
from test_gpu_pose_vertices import bits, matrices, moved, oracle_moved, overflows
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, first_difference, frame, oracle_frame, same, scene
from test_skin_cpu import PALETTE_SIZES, bindings, case, palette_of, rest_of
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError, make_bones

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = abi.SKIN_LDS_BONES
# (palette size, knob skin_no_lds): both values where the palette fits the LDS bound, so that both kernels see the same input
VARIANTS = [(nb, knob) for nb in PALETTE_SIZES for knob in ((0, 1) if nb <= LDS else (0,))]


def small_case(residence, which=0, n_bones=3, seed=11):
    """(first, bones_idx, weights, palette) of the residence's first (ragged) or second (whole) binding"""
    first, count = bindings(residence)[which]
    b, w = sr.binding(count, n_bones, seed)
    return first, b, w, palette_of(residence, n_bones)


def bind_and_skin(t, first, b, w, palette):
    t.skin_bind(b, w, first=first)
    t.skin_vertices(palette)


def one_hot(count, bone_of):
    """influences (1, 0, 0, 0) with bone_of[i] under the 1 and other valid bones under the zeros"""
    b = np.zeros((count, 4), np.int64)
    b[:, 0] = bone_of
    b[:, 1:] = [1, 0, 1]
    w = np.zeros((count, 4), F)
    w[:, 0] = 1
    return b, w


# --------------------------------------------------------------------------------------------------- vertices
@pytest.mark.parametrize("n_bones,no_lds", VARIANTS)
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_skinned_vertices_are_the_definition_s(gpu, residence, which, n_bones, no_lds):
    v0 = rest_of(residence)
    first, count = bindings(residence)[which]
    b, w, palette = case(residence, first, count, n_bones)
    assert sr.valid_binding(first, b, w, len(v0)) and sr.valid_palette(palette, b.max())
    gpu.upload_scene(scene(residence).view)
    gpu.debug_set("skin_no_lds", no_lds)
    try:
        gpu.skin_bind(b, w, first=first)
        assert np.array_equal(bits(gpu.download_vertices()), bits(v0))                   # a bind alone moves no vertex
        gpu.skin_vertices(palette)
        got, want = gpu.download_vertices(), sr.skin(v0, v0, first, b, w, palette)
    finally:
        gpu.debug_set("skin_no_lds", 0)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} vertices differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    m = np.zeros(len(v0), bool)
    m[first:first + count] = True
    assert np.array_equal(bits(got[~m]), bits(v0[~m])) and (bits(got[m]) != bits(v0[m])).any(axis=1).all()
    assert gpu.pose_overflows() == 0


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_one_hot_influences_equal_a_pose(gpu, residence):
    sc, v0 = scene(residence), rest_of(residence)
    first, count = bindings(residence)[0]
    half = count // 2
    a, b_ = matrices(residence, "A"), matrices(residence, "B")
    idx, w = one_hot(count, np.arange(count) >= half)
    gpu.upload_scene(sc.view)
    bind_and_skin(gpu, first, idx, w, [a, b_])
    skinned, skinned_frame = gpu.download_vertices(), frame(gpu, 4, MIS)
    with Tracer(0) as posed:
        posed.upload_scene(sc.view)
        posed.pose_vertices([(first, half, *a), (first + half, count - half, *b_)])
        want = posed.download_vertices()
        assert (skinned == want).all() and not np.array_equal(bits(want), bits(v0))      # as values: a -0 may be a +0
        assert same(frame(posed, 4, MIS), skinned_frame)


# --------------------------------------------------------------------------------------------------- tree
@pytest.mark.parametrize("tree", ["sah_triangle_leaves", "lbvh"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_downloaded_tree_is_the_refit_of_the_tree_before(gpu, residence, tree):
    sc = scene(residence)
    if tree == "lbvh":
        gpu.upload_scene_lbvh(sc.leaves_view())
    else:
        gpu.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    before = rr.raw(gpu.download_bvh())
    v0, idx = rest_of(residence), rr.indices_of(sc.view)
    current = v0
    for which, n_bones, seed in ((0, 3, 11), (1, LDS + 1, 12), (0, 5, 13)):
        first, b, w, palette = small_case(residence, which, n_bones, seed)
        bind_and_skin(gpu, first, b, w, palette)
        current = sr.skin(v0, current, first, b, w, palette)
        got = rr.raw(gpu.download_bvh())
        assert not first_difference(got, rr.refit(before, current, idx)), (which, n_bones)
    assert (got[:, :8] == before[:, :8]).all()                       # links, axis, pType, pIndex: the topology stays


@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_both_refit_variants_give_the_definition_s_bits(tracer, residence):
    """twice, so that a counter the single launch did not put back shows in the second result"""
    sc, v0 = scene(residence), rest_of(residence)
    tracer.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    before = rr.raw(tracer.download_bvh())
    current = v0
    for seed in (11, 12):
        first, b, w, palette = small_case(residence, 0, 3, seed)
        bind_and_skin(tracer, first, b, w, palette)
        current = sr.skin(v0, current, first, b, w, palette)
        assert not first_difference(rr.raw(tracer.download_bvh()), rr.refit(before, current, rr.indices_of(sc.view))), seed
    m = rr.Moved(sc.view, rr.raw(tracer.download_bvh()), current)
    assert same(frame(tracer, 4, PATH), oracle_frame(m.view, 4, PATH))


# --------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("integrator", [PATH, MIS])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_frame_after_skin_is_the_oracle_s_and_the_update_s(gpu, residence, integrator):
    sc, v0 = scene(residence), rest_of(residence)
    first, b, w, palette = small_case(residence)
    v = sr.skin(v0, v0, first, b, w, palette)
    gpu.upload_scene(sc.view)
    original = frame(gpu, 4, integrator)
    bind_and_skin(gpu, first, b, w, palette)
    got = frame(gpu, 4, integrator)
    assert same(got, oracle_moved(residence, v, 4, integrator))
    assert not same(got, original)
    with Tracer(0) as fresh:                                            # ... and what the host's own arithmetic, passed in, gives
        fresh.upload_scene(sc.view)
        fresh.update_vertices(v)
        assert same(frame(fresh, 4, integrator), got)


# --------------------------------------------------------------------------------------------------- always from rest
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_a_skin_is_applied_to_the_rest_vertices(gpu, residence):
    sc, v0 = scene(residence), rest_of(residence)
    n = len(v0)
    first, b, w, pal_a = small_case(residence)
    count = len(b)
    pal_b = sr.palette(5, pr.box_centre(v0))[2:]
    gpu.upload_scene(sc.view)                                           # no pose came before: the first skin makes the rest copy
    bind_and_skin(gpu, first, b, w, pal_a)
    gpu.skin_vertices(pal_b)
    after_ab, frame_ab = gpu.download_vertices(), frame(gpu, 4, PATH)
    with Tracer(0) as fresh:                                            # A then B is B on a fresh upload
        fresh.upload_scene(sc.view)
        bind_and_skin(fresh, first, b, w, pal_b)
        assert np.array_equal(bits(fresh.download_vertices()), bits(after_ab)) and same(frame(fresh, 4, PATH), frame_ab)
    want = sr.skin(v0, v0, first, b, w, pal_b)
    assert np.array_equal(bits(after_ab), bits(want)) and not np.array_equal(bits(want), bits(sr.skin(v0, v0, first, b, w, pal_a)))
    # a pose that overlaps the binding on both sides: the next skin overwrites the bound vertices from rest and keeps the pose outside
    p_first = max(first - 2, 0)
    poses = [(p_first, min(count // 2, n - p_first), *matrices(residence, "A"))]
    gpu.pose_vertices(poses)
    posed = pr.pose(v0, want, poses)
    assert np.array_equal(bits(gpu.download_vertices()), bits(posed))
    gpu.skin_vertices(pal_a)
    want = sr.skin(v0, posed, first, b, w, pal_a)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))
    assert np.array_equal(bits(want[first:first + count]), bits(sr.skin(v0, v0, first, b, w, pal_a)[first:first + count]))
    if first > 0:
        assert np.array_equal(bits(want[p_first:first]), bits(posed[p_first:first])) and not np.array_equal(bits(want[p_first:first]), bits(v0[p_first:first]))
    # an update of part of the range moves the rest vertices of that part
    lo, hi = first + 2, first + count - 1
    rest = v0.copy()
    rest[lo:hi] = rr.twist(v0, 0.4, 0.8)[lo:hi]
    gpu.update_vertices(rest[lo:hi], first=lo)
    current = want.copy(); current[lo:hi] = rest[lo:hi]
    assert np.array_equal(bits(gpu.download_vertices()), bits(current))
    gpu.skin_vertices(pal_a)
    want2 = sr.skin(rest, current, first, b, w, pal_a)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want2)) and not np.array_equal(bits(want2), bits(want))
    assert same(frame(gpu, 4, PATH), oracle_moved(residence, want2, 4, PATH))


# --------------------------------------------------------------------------------------------------- state carried across
def test_triangle_materials_survive(gpu):
    from test_gpu_triangle_materials import Relabelled
    from conftest import random_rays
    sc, v0 = scene("mem"), rest_of("mem")
    first, b, w, palette = small_case("mem")
    rel = Relabelled(sc.view)
    gpu.upload_scene(rel.view(sc.view))
    gpu.upload_triangle_materials(np.full(sc.view.n_index // 3, rel.k, np.uint32))
    bind_and_skin(gpu, first, b, w, palette)
    assert same(frame(gpu, 4, MIS), oracle_moved("mem", sr.skin(v0, v0, first, b, w, palette), 4, MIS))
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 50 and (hits["material"][tri] == rel.k).all()
    gpu.upload_triangle_materials(None)


def test_mesh_light_tables_follow_the_skin():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "meshlight_ref"))
    import meshlight_loader as ml
    ref = ml.build()
    sc, v0 = scene("lds"), rest_of("lds")
    n = sc.view.n_index // 3
    tri_mat = np.full(n, 4, np.uint32); tri_mat[n // 2:n // 2 + 6] = 3   # Cornell's table: 3 = the lamp's emitter, 4 = the red Lambert
    grow = pr.turn(pr.box_centre(v0), 0.3, (1.4, 1.4, 1.4))              # the emissive triangles grow
    idx, w = one_hot(len(v0), 0)
    w[:, 1] = F(0.25)                                                    # 1.25 times the two bones' blend: not a pose
    with Tracer(0, hooks=True) as t:
        t.upload_scene(sc.view)
        t.upload_triangle_materials(tri_mat)
        before = t.mesh_light_tables(n)
        bind_and_skin(t, 0, idx, w, [grow, grow])
        g = t.mesh_light_tables(n)
        m = rr.Moved(sc.view, sc.bvh_array().copy(), sr.skin(v0, v0, 0, idx, w, [grow, grow]))
        c = ref.tables(ml.view_triangles(m.view), tri_mat, *ml.view_materials(m.view))
        assert g["n_lights"] == c["n_lights"] == before["n_lights"] > 0
        assert np.array_equal(g["tri"], c["tri"]) and np.array_equal(g["alias"], c["alias"])
        assert np.array_equal(g["pdfA"].view(np.uint32), c["pdfA"].view(np.uint32)) and g["total"] == c["total"]
        assert g["total"] > before["total"]


def test_gbuffer_shows_the_new_depth(gpu):
    sc, v0 = scene("lds"), rest_of("lds")
    shrink = pr.turn(pr.box_centre(v0), 0.0, (0.5, 0.5, 0.5))            # the ball shrinks to half its size
    idx, w = one_hot(len(v0), 0)
    gpu.upload_scene(sc.view)
    frame(gpu, 2, PATH)
    gpu.denoise()
    before = gpu.download_gbuffer()
    bind_and_skin(gpu, 0, idx, w, [shrink, shrink])
    frame(gpu, 2, PATH)
    gpu.denoise()
    after = gpu.download_gbuffer()
    with Tracer(0) as fresh:
        m = moved("lds", sr.skin(v0, v0, 0, idx, w, [shrink, shrink]))
        fresh.upload_scene(m.view)
        frame(fresh, 2, PATH)
        fresh.denoise()
        want = fresh.download_gbuffer()
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()


def test_block_costs_are_kept_and_move_no_pixel(gpu):
    v0 = rest_of("mem")
    small = pr.turn(pr.box_centre(v0), 0.2, (0.9, 0.9, 0.9))
    idx, w = one_hot(len(v0), 0)
    gpu.upload_scene(scene("mem").view)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    bind_and_skin(gpu, 0, idx, w, [small, small])
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)  # the costs were kept ...
    ordered = frame(gpu, 16, PATH)
    gpu.skin_vertices([small, small])
    assert same(frame(gpu, 16, PATH, fixed_order=True), ordered)        # ... and order is scheduling only
    assert same(ordered, oracle_moved("mem", sr.skin(v0, v0, 0, idx, w, [small, small]), 16, PATH))


# --------------------------------------------------------------------------------------------------- the binding's lifetime
def test_binding_lifetime(gpu):
    sc, v0 = scene("lds"), rest_of("lds")
    n = len(v0)
    first, b, w, palette = small_case("lds")
    gpu.upload_scene(sc.view)
    bind_and_skin(gpu, first, b, w, palette)
    # a rebind replaces the binding: the old range keeps its skinned values, the new one is computed from rest
    b2, w2 = sr.binding(4, 3, seed=21)
    gpu.skin_bind(b2, w2, first=1)
    gpu.skin_vertices(palette)
    want = sr.skin(v0, sr.skin(v0, v0, first, b, w, palette), 1, b2, w2, palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))
    # update_vertices, pose_vertices and upload_triangle_materials keep it
    rest = v0.copy()
    rest[2:4] = rr.twist(v0, 0.3, 0.9)[2:4]
    gpu.update_vertices(rest[2:4], first=2)
    gpu.pose_vertices([(0, 3, *matrices("lds", "B"))])
    gpu.upload_triangle_materials(np.full(sc.view.n_index // 3, 4, np.uint32))
    current = gpu.download_vertices()
    gpu.skin_vertices(palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(sr.skin(rest, current, 1, b2, w2, palette)))
    gpu.upload_triangle_materials(None)
    # count == 0 unbinds
    verts = gpu.download_vertices()
    gpu.skin_bind(b[:0], w[:0])
    with pytest.raises(TracerError) as e:
        gpu.skin_vertices(palette)
    assert e.value.status == abi.ERR_INVALID_ARG
    assert gpu._L.trc_skin_bind(gpu._h, None, 0, 0) == abi.OK            # influences may be NULL with count == 0
    assert np.array_equal(bits(gpu.download_vertices()), bits(verts))
    # an upload drops the binding
    gpu.skin_bind(b, w, first=first)
    gpu.upload_scene(sc.view)
    with pytest.raises(TracerError) as e:
        gpu.skin_vertices(palette)
    assert e.value.status == abi.ERR_INVALID_ARG
    assert np.array_equal(bits(gpu.download_vertices()), bits(v0)) and n == len(v0)


# --------------------------------------------------------------------------------------------------- refusals, overflow
def test_refusals_change_nothing(gpu):
    i = pr.identity()
    with Tracer(0) as fresh:
        b1, w1 = one_hot(1, 0)
        with pytest.raises(TracerError) as e:
            fresh.skin_bind(b1, w1)
        assert e.value.status == abi.ERR_NO_SCENE
        with pytest.raises(TracerError) as e:
            fresh.skin_vertices([(i, i), (i, i)])
        assert e.value.status == abi.ERR_NO_SCENE
        spheres = host.HostScene(abi.SCENE_CORNELL_SPHERES)                        # a scene without triangles; kept alive: its view
        fresh.upload_scene(spheres.view)                                           # points into memory the scene owns
        fresh.skin_vertices([])                                                    # n_bones == 0 without a binding: TRC_OK
        assert fresh._L.trc_skin_vertices(fresh._h, None, 0) == abi.OK
        for call in (lambda: fresh.skin_bind(b1, w1), lambda: fresh.skin_vertices([(i, i), (i, i)])):
            with pytest.raises(TracerError) as e:
                call()
            assert e.value.status == abi.ERR_INVALID_ARG
    sc, v0 = scene("lds"), rest_of("lds")
    n = len(v0)
    first, b, w, palette = small_case("lds")
    count = len(b)
    gpu.upload_scene(sc.view)
    bind_and_skin(gpu, first, b, w, palette)                                      # refusals on a context that has skinned once
    verts, before = gpu.download_vertices(), frame(gpu, 4, MIS)

    def unchanged():
        assert np.array_equal(bits(gpu.download_vertices()), bits(verts))
        assert same(frame(gpu, 4, MIS), before)

    # ---- trc_skin_bind
    w_nan, w_inf, b_big = w.copy(), w.copy(), b.copy()
    w_nan[2, 1] = np.nan; w_inf[count - 1, 3] = -np.inf; b_big[1, 2] = abi.TRC_SKIN_MAX_BONES
    refused = [(first + 6, b, w), (n, b[:1], w[:1]), (0xFFFFFFFF, b[:2], w[:2]), (first, b, w_nan), (first, b, w_inf), (first, b_big, w)]
    for f, bb, ww in refused:
        assert not sr.valid_binding(f, bb, ww, n)
        with pytest.raises(TracerError) as e:
            gpu.skin_bind(bb, ww, first=f)
        assert e.value.status == abi.ERR_INVALID_ARG, (f, len(bb))
        unchanged()
    table = np.zeros((4, 8), np.uint32)
    table[:, 4:] = np.ones((4, 4), F).view(np.uint32)
    assert gpu._L.trc_skin_bind(gpu._h, None, 0, 2) == abi.ERR_INVALID_ARG                          # NULL with a count
    assert gpu._L.trc_skin_bind(gpu._h, table.ctypes.data, 2, 0xFFFFFFFF) == abi.ERR_INVALID_ARG    # first + count wraps
    unchanged()
    gpu.skin_vertices(palette)                                                    # a refused rebind leaves the old binding working
    unchanged()
    # ---- trc_skin_vertices
    nan, inf, nan_n, inf_n = palette[1][0].copy(), palette[0][0].copy(), palette[2][1].copy(), palette[1][1].copy()
    nan[2, 3] = np.nan; inf[0, 0] = -np.inf; nan_n[0, 2] = np.nan; inf_n[2, 1] = np.inf
    assert b.max() == 2
    refused = [palette[:2],                                                                        # n_bones one too small
               [palette[0], (nan, palette[1][1]), palette[2]], [(inf, palette[0][1])] + palette[1:],
               palette[:2] + [(palette[2][0], nan_n)], [palette[0], (palette[1][0], inf_n), palette[2]],
               palette + [(nan, i)]]                                                               # a bone that no vertex names
    for pal in refused:
        assert not sr.valid_palette(pal, b.max())
        with pytest.raises(TracerError) as e:
            gpu.skin_vertices(pal)
        assert e.value.status == abi.ERR_INVALID_ARG, len(pal)
        unchanged()
    assert gpu._L.trc_skin_vertices(gpu._h, None, 3) == abi.ERR_INVALID_ARG
    assert gpu._L.trc_skin_vertices(gpu._h, make_bones(palette), abi.TRC_SKIN_MAX_BONES + 1) == abi.ERR_INVALID_ARG
    unchanged()
    gpu.skin_vertices([])                                                         # n_bones == 0 with a binding: TRC_OK, nothing happens
    assert gpu._L.trc_skin_vertices(gpu._h, None, 0) == abi.OK
    unchanged()
    # what is not read may hold anything
    dirty = []
    for model, normal in palette:
        model, normal = model.copy(), normal.copy()
        model[3, :] = np.nan; normal[3, :] = np.nan; normal[:, 3] = np.inf
        dirty.append((model, normal))
    assert sr.valid_palette(dirty, b.max())
    gpu.skin_vertices(dirty)
    unchanged()
    gpu.skin_bind(b[:0], w[:0])
    with pytest.raises(TracerError) as e:                                         # no binding
        gpu.skin_vertices(palette)
    assert e.value.status == abi.ERR_INVALID_ARG
    unchanged()


def test_overflow_is_counted_and_an_identity_palette_restores(gpu):
    """The count is the definition's: skinned positions that are not finite or beyond 1e37.  As in the pose's test, bones of scale 1e30
    leave every position of the Cornell scene near 1e32, inside the bound (count 0); 1e36 takes all nine bound vertices past it.
    Nothing is rendered between an overflow and the skin that undoes it."""
    v0 = rest_of("lds")
    i = pr.identity()
    idx, w = one_hot(9, np.arange(9) % 2)
    gpu.upload_scene(scene("lds").view)
    gpu.skin_bind(idx, w, first=2)
    assert gpu.pose_overflows() == 0
    for scale in (1e30, 1e36):
        huge = [(i * F(scale), i)] * 2
        gpu.skin_vertices(huge)
        with np.errstate(all="ignore"):
            want = overflows(sr.skin(v0, v0, 2, idx, w, huge)[2:11, :3])
        assert gpu.pose_overflows() == want, scale
    assert want == 9 and np.abs(v0[2:11, :3]).max() * 1e30 < 1e37
    gpu.skin_vertices(sr.identity_palette(2))
    assert gpu.pose_overflows() == 0
    got = gpu.download_vertices()
    assert (got == v0).all()                                                     # as values: a -0 may have become +0
    assert same(frame(gpu, 4, PATH), oracle_moved("lds", got, 4, PATH))


# --------------------------------------------------------------------------------------------------- the example host
def test_example_host_bend(tmp_path):
    """examples/trc_render --bend 2 on a tetrahedron: trc_skin_bind once and trc_skin_vertices per frame through the C ABI only"""
    obj, out = tmp_path / "tet.obj", tmp_path / "f.png"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 3 2\nf 1 2 4\nf 2 3 4\nf 1 4 3\n")
    r = subprocess.run([os.path.join(ROOT, "examples", "trc_render"), "--mesh", str(obj), "--size", "48", "32", "--spp", "2", "--bend", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("trc_skin_vertices") == 2
    frames = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (1, 2)]
    assert frames[0].shape == frames[1].shape == host.load_png(out).shape
    assert not np.array_equal(frames[0], frames[1])                              # half a bend and a whole turn of the top
