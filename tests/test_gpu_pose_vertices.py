"""trc_pose_vertices on the GPU (include/tracer_abi.h): the posed vertices against the definition (tests/pose_ref.py) bit for bit, and
everything behind them -- tree, frames, what is kept and what is dropped -- against what trc_update_vertices leaves for the same
vertices, against the definition of the refit (tests/refit_ref.py) and against the CPU oracle.  The range tables put lane, wavefront
and 256-thread boundaries inside ranges and between them, and come unsorted."""
import os
import subprocess

import numpy as np
import pytest

import pose_ref as pr
import refit_ref as rr
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, first_difference, frame, oracle_frame, same, scene
from test_pose_cpu import ANGLE_A, ANGLE_B, SCALE_A, SCALE_B, SHIFT_A, SHIFT_B
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rest_of(residence):
    return rr.vertices_of(scene(residence).view)


def matrices(residence, which):
    angle, scale, shift = {"A": (ANGLE_A, SCALE_A, SHIFT_A), "B": (ANGLE_B, SCALE_B, SHIFT_B)}[which]
    return pr.turn(pr.box_centre(rest_of(residence)), angle, scale, shift)


def table(residence, name, which="AB"):
    """[(first, count, model, normal)], NOT sorted by first; `which`: the matrices the ranges take in turn"""
    n = len(rest_of(residence))
    ranges = {
        # counts 1, 63 and 257 back to back (ends at 1, 64 and 321: a lane, a wavefront, and past a 256-thread block), a gap, and a
        # last range that ends exactly at n_vertex
        ("mem", "ragged"): [(64, 257), (400, n - 400), (0, 1), (1, 63)],
        ("mem", "whole"): [(0, n)],
        ("lds", "ragged"): [(n - 9, 7), (0, 5), (5, 11)],            # [16, n - 9) and the last two vertices are in no range
        ("lds", "whole"): [(0, n)],
    }[(residence, name)]
    return [(f, c, *matrices(residence, which[k % len(which)])) for k, (f, c) in enumerate(ranges)]


def moved(residence, v):
    """the scene over refit() of the host tree and the vertices v; the caller keeps the object for as long as it uses its .view"""
    sc = scene(residence)
    return rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)


def oracle_moved(residence, v, spp, integrator):
    m = moved(residence, v)
    return oracle_frame(m.view, spp, integrator)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def touched(poses, n):
    m = np.zeros(n, bool)
    for f, c, _, _ in poses:
        m[f:f + c] = True
    return m


# --------------------------------------------------------------------------------------------------- vertices
@pytest.mark.parametrize("residence,name", [("mem", "ragged"), ("mem", "whole"), ("lds", "ragged"), ("lds", "whole")])
def test_posed_vertices_are_the_definition_s(gpu, residence, name):
    v0 = rest_of(residence)
    assert len(v0) > 700 if residence == "mem" else len(v0) > 18
    gpu.upload_scene(scene(residence).view)
    assert np.array_equal(bits(gpu.download_vertices()), bits(v0))
    assert np.array_equal(bits(gpu.download_vertices(3, 7)), bits(v0[3:10]))
    poses = table(residence, name)
    assert pr.valid(poses, len(v0))
    assert len(poses) == 1 or [p[0] for p in poses] != sorted(p[0] for p in poses)
    gpu.pose_vertices(poses)
    got, want = gpu.download_vertices(), pr.pose(v0, v0, poses)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} vertices differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    m = touched(poses, len(v0))
    assert np.array_equal(bits(got[~m]), bits(v0[~m])) and (bits(got[m]) != bits(v0[m])).any(axis=1).all()
    assert gpu.pose_overflows() == 0


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
    for name, which in (("ragged", "AB"), ("whole", "B"), ("ragged", "BA")):
        poses = table(residence, name, which)
        gpu.pose_vertices(poses)
        current = pr.pose(v0, current, poses)
        got = rr.raw(gpu.download_bvh())
        assert not first_difference(got, rr.refit(before, current, idx)), (name, which)
    assert (got[:, :8] == before[:, :8]).all()                       # links, axis, pType, pIndex: the topology stays


# --------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("integrator", [PATH, MIS])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_frame_after_pose_is_the_oracle_s_and_the_update_s(gpu, residence, integrator):
    sc, v0 = scene(residence), rest_of(residence)
    poses = table(residence, "ragged")
    v = pr.pose(v0, v0, poses)
    gpu.upload_scene(sc.view)
    original = frame(gpu, 4, integrator)
    gpu.pose_vertices(poses)
    got = frame(gpu, 4, integrator)
    assert same(got, oracle_moved(residence, v, 4, integrator))
    assert not same(got, original)
    with Tracer(0) as fresh:                                            # ... and what the host's own arithmetic, passed in, gives
        fresh.upload_scene(sc.view)
        fresh.update_vertices(v)
        assert same(frame(fresh, 4, integrator), got)


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
    for which in ("AB", "BA"):
        poses = table(residence, "ragged", which)
        tracer.pose_vertices(poses)
        current = pr.pose(v0, current, poses)
        assert not first_difference(rr.raw(tracer.download_bvh()), rr.refit(before, current, rr.indices_of(sc.view))), which
    m = rr.Moved(sc.view, rr.raw(tracer.download_bvh()), current)
    assert same(frame(tracer, 4, PATH), oracle_frame(m.view, 4, PATH))


# --------------------------------------------------------------------------------------------------- no drift
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_a_pose_is_applied_to_the_rest_vertices(gpu, residence):
    sc, v0 = scene(residence), rest_of(residence)
    n = len(v0)
    a, b = table(residence, "ragged", "A"), table(residence, "ragged", "B")
    gpu.upload_scene(sc.view)
    gpu.pose_vertices(a)
    gpu.pose_vertices(b)
    after_ab, frame_ab = gpu.download_vertices(), frame(gpu, 4, PATH)
    with Tracer(0) as fresh:                                            # A then B is B on a fresh upload
        fresh.upload_scene(sc.view)
        fresh.pose_vertices(b)
        assert np.array_equal(bits(fresh.download_vertices()), bits(after_ab)) and same(frame(fresh, 4, PATH), frame_ab)
    assert np.array_equal(bits(after_ab), bits(pr.pose(v0, v0, b)))
    # an update of a sub-range moves the rest vertices of that sub-range: the same pose again is the pose of the updated rest array
    lo, hi = a[0][0] + 2, a[0][0] + a[0][1] - 1                         # inside the first range of the table
    rest = v0.copy()
    rest[lo:hi] = rr.twist(v0, 0.4, 0.8)[lo:hi]
    gpu.update_vertices(rest[lo:hi], first=lo)
    current = after_ab.copy(); current[lo:hi] = rest[lo:hi]
    assert np.array_equal(bits(gpu.download_vertices()), bits(current))
    gpu.pose_vertices(b)
    want = pr.pose(rest, current, b)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want)) and not np.array_equal(bits(want), bits(after_ab))
    assert same(frame(gpu, 4, PATH), oracle_moved(residence, want, 4, PATH))
    # a call that names one of the ranges leaves the others as the call before posed them
    gpu.pose_vertices(a[1:2])
    want2 = pr.pose(rest, want, a[1:2])
    assert np.array_equal(bits(gpu.download_vertices()), bits(want2)) and not np.array_equal(bits(want2), bits(want))
    assert same(frame(gpu, 4, PATH), oracle_moved(residence, want2, 4, PATH))
    assert n == len(want2)


# --------------------------------------------------------------------------------------------------- state carried across
def test_triangle_materials_survive(gpu):
    from test_gpu_triangle_materials import Relabelled
    from conftest import random_rays
    sc, v0 = scene("mem"), rest_of("mem")
    rel = Relabelled(sc.view)
    gpu.upload_scene(rel.view(sc.view))
    gpu.upload_triangle_materials(np.full(sc.view.n_index // 3, rel.k, np.uint32))
    poses = table("mem", "ragged")
    gpu.pose_vertices(poses)
    assert same(frame(gpu, 4, MIS), oracle_moved("mem", pr.pose(v0, v0, poses), 4, MIS))
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 50 and (hits["material"][tri] == rel.k).all()
    gpu.upload_triangle_materials(None)


def test_mesh_light_tables_follow_the_pose():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "meshlight_ref"))
    import meshlight_loader as ml
    ref = ml.build()
    sc, v0 = scene("lds"), rest_of("lds")
    n = sc.view.n_index // 3
    tri_mat = np.full(n, 4, np.uint32); tri_mat[n // 2:n // 2 + 6] = 3   # Cornell's table: 3 = the lamp's emitter, 4 = the red Lambert
    grow, grow_n = pr.turn(pr.box_centre(v0), 0.3, (1.4, 1.4, 1.4))      # the emissive triangles grow
    with Tracer(0, hooks=True) as t:
        t.upload_scene(sc.view)
        t.upload_triangle_materials(tri_mat)
        before = t.mesh_light_tables(n)
        poses = [(0, len(v0), grow, grow_n)]
        t.pose_vertices(poses)
        g = t.mesh_light_tables(n)
        m = rr.Moved(sc.view, sc.bvh_array().copy(), pr.pose(v0, v0, poses))
        c = ref.tables(ml.view_triangles(m.view), tri_mat, *ml.view_materials(m.view))
        assert g["n_lights"] == c["n_lights"] == before["n_lights"] > 0
        assert np.array_equal(g["tri"], c["tri"]) and np.array_equal(g["alias"], c["alias"])
        assert np.array_equal(g["pdfA"].view(np.uint32), c["pdfA"].view(np.uint32)) and g["total"] == c["total"]
        assert g["total"] > before["total"]


def test_gbuffer_shows_the_new_depth(gpu):
    sc, v0 = scene("lds"), rest_of("lds")
    poses = [(0, len(v0), *pr.turn(pr.box_centre(v0), 0.0, (0.5, 0.5, 0.5)))]      # the ball shrinks to half its size
    gpu.upload_scene(sc.view)
    frame(gpu, 2, PATH)
    gpu.denoise()
    before = gpu.download_gbuffer()
    gpu.pose_vertices(poses)
    frame(gpu, 2, PATH)
    gpu.denoise()
    after = gpu.download_gbuffer()
    with Tracer(0) as fresh:
        m = moved("lds", pr.pose(v0, v0, poses))
        fresh.upload_scene(m.view)
        frame(fresh, 2, PATH)
        fresh.denoise()
        want = fresh.download_gbuffer()
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()


def test_block_costs_are_kept_and_move_no_pixel(gpu):
    v0 = rest_of("mem")
    poses = [(0, len(v0), *pr.turn(pr.box_centre(v0), 0.2, (0.9, 0.9, 0.9)))]
    gpu.upload_scene(scene("mem").view)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    gpu.pose_vertices(poses)
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)  # the costs were kept ...
    ordered = frame(gpu, 16, PATH)
    gpu.pose_vertices(poses)
    assert same(frame(gpu, 16, PATH, fixed_order=True), ordered)        # ... and order is scheduling only
    assert same(ordered, oracle_moved("mem", pr.pose(v0, v0, poses), 16, PATH))


# --------------------------------------------------------------------------------------------------- refusals, overflow
def test_refusals_change_nothing(gpu):
    i = pr.identity()
    with Tracer(0) as fresh:
        with pytest.raises(TracerError) as e:
            fresh.pose_vertices([(0, 1, i, i)])
        assert e.value.status == abi.ERR_NO_SCENE
        with pytest.raises(TracerError) as e:
            fresh.download_vertices(0, 1)
        assert e.value.status == abi.ERR_NO_SCENE
        spheres = host.HostScene(abi.SCENE_CORNELL_SPHERES)                      # a scene without triangles
        fresh.upload_scene(spheres.view)
        fresh.pose_vertices([])
        for call in (lambda: fresh.pose_vertices([(0, 1, i, i)]), lambda: fresh.download_vertices(0, 0)):
            with pytest.raises(TracerError) as e:
                call()
            assert e.value.status == abi.ERR_INVALID_ARG
    sc, v0 = scene("lds"), rest_of("lds")
    n = len(v0)
    a, _ = matrices("lds", "A")
    gpu.upload_scene(sc.view)
    gpu.pose_vertices(table("lds", "ragged"))                                    # refusals after a pose: the rest copy exists
    verts, before = gpu.download_vertices(), frame(gpu, 4, MIS)
    nan, inf, nan_n, inf_n = a.copy(), a.copy(), i.copy(), i.copy()
    nan[2, 3] = np.nan; inf[0, 0] = -np.inf; nan_n[0, 2] = np.nan; inf_n[2, 1] = np.inf
    refused = [[(0, 0, a, i)], [(0, 4, a, i), (7, 0, a, i)],                     # count == 0
               [(1, n, a, i)], [(n, 1, a, i)], [(n - 1, 2, a, i)], [(0xFFFFFFFF, 2, a, i)], [(2, 0xFFFFFFFF, a, i)],   # past n_vertex
               [(0, 5, a, i), (4, 2, a, i)], [(6, 3, a, i), (0, 7, a, i)], [(2, 3, a, i), (2, 3, a, i)], [(0, n, a, i), (3, 1, a, i)],   # overlap
               [(0, n, nan, i)], [(0, n, inf, i)], [(0, n, a, nan_n)], [(0, 3, a, i), (3, 3, a, inf_n)]]                 # not finite
    for poses in refused:
        assert not pr.valid(poses, n)
        with pytest.raises(TracerError) as e:
            gpu.pose_vertices(poses)
        assert e.value.status == abi.ERR_INVALID_ARG, poses
        assert np.array_equal(bits(gpu.download_vertices()), bits(verts))
        assert same(frame(gpu, 4, MIS), before)
    assert gpu._L.trc_pose_vertices(gpu._h, None, 2) == abi.ERR_INVALID_ARG
    for first, count in ((1, n), (n, 1), (0xFFFFFFFF, 2)):
        with pytest.raises(TracerError) as e:
            gpu.download_vertices(first, count)
        assert e.value.status == abi.ERR_INVALID_ARG
    assert gpu._L.trc_download_vertices(gpu._h, None, 0, 2) == abi.ERR_INVALID_ARG
    # what is not read may hold anything
    unread, unread_n = a.copy(), i.copy()
    unread[3, :] = np.nan; unread_n[3, :] = np.nan; unread_n[:, 3] = np.inf
    assert pr.valid([(0, n, unread, unread_n)], n)
    gpu.pose_vertices([(0, n, unread, unread_n)])
    assert np.array_equal(bits(gpu.download_vertices()), bits(pr.pose(v0, v0, [(0, n, a, i)])))
    gpu.pose_vertices(table("lds", "ragged"))
    gpu.pose_vertices(table("lds", "whole", "A")[:0])                            # n_poses == 0: TRC_OK, nothing happens
    assert gpu._L.trc_pose_vertices(gpu._h, None, 0) == abi.OK
    assert len(gpu.download_vertices(n, 0)) == 0
    want = pr.pose(v0, pr.pose(v0, v0, [(0, n, a, i)]), table("lds", "ragged"))
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))


def overflows(positions):
    return int((~(np.abs(positions) <= F(1e37))).any(axis=1).sum())


def test_overflow_is_counted_and_an_identity_pose_restores(gpu):
    """The count is the definition's: posed positions that are not finite or beyond 1e37.  The Cornell scene's coordinates are a few
    hundred at most, so a scale of 1e30 leaves every position near 1e32, inside the bound, and the count the definition gives for it
    is 0; 1e36 takes the same range past the bound (1e38 and more, some of it infinite).  Nothing is rendered between an overflow and
    the pose that undoes it."""
    v0 = rest_of("lds")
    i = pr.identity()
    gpu.upload_scene(scene("lds").view)
    assert gpu.pose_overflows() == 0
    for scale in (1e30, 1e36):
        huge = i * F(scale)
        gpu.pose_vertices([(2, 9, huge, i)])
        with np.errstate(over="ignore"):
            want = overflows(pr.pose(v0, v0, [(2, 9, huge, i)])[2:11, :3])
        assert gpu.pose_overflows() == want, scale
    assert want == 9 and np.abs(v0[2:11, :3]).max() * 1e30 < 1e37
    gpu.pose_vertices([(2, 9, i, i)])
    assert gpu.pose_overflows() == 0
    got = gpu.download_vertices()
    assert (got == v0).all()                                                     # as values: a -0 may have become +0
    assert same(frame(gpu, 4, PATH), oracle_moved("lds", got, 4, PATH))


# --------------------------------------------------------------------------------------------------- the example host
def test_example_host_pose(tmp_path):
    """examples/trc_render --pose 2 on a tetrahedron: trc_pose_vertices through the C ABI only, one PNG per posed frame"""
    obj, out = tmp_path / "tet.obj", tmp_path / "f.png"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 3 2\nf 1 2 4\nf 2 3 4\nf 1 4 3\n")
    r = subprocess.run([os.path.join(ROOT, "examples", "trc_render"), "--mesh", str(obj), "--size", "48", "32", "--spp", "2", "--pose", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("trc_pose_vertices") == 2
    frames = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (1, 2)]
    assert frames[0].shape == frames[1].shape == host.load_png(out).shape
    assert not np.array_equal(frames[0], frames[1])                              # half a turn and a whole one
