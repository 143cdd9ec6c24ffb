"""trc_recompute_normals on the GPU (include/tracer_abi.h): the re-derived normals against the definition (tests/normals_ref.py) bit for
bit -- on the two balls of the other animation tests and on normals_ref.fan (a hub of valence 70, a vertex without a corner, triangles
without area, half a rim wound against its normals), over the ragged and the whole range of tests/test_skin_cpu.py, after every upload
path -- and everything behind them against what trc_update_vertices leaves for the same vertices and against the CPU oracle: frames,
the G-buffer, what is kept and what is dropped, the adjacency's lifetime, refusals that change nothing."""
import os
import subprocess

import numpy as np
import pytest

import morph_ref as mr
import normals_ref as nr
import pose_ref as pr
import refit_ref as rr
import skin_ref as sr
from test_gpu_morph_vertices import layouts
from test_gpu_pose_vertices import bits, oracle_moved
from test_gpu_pose_vertices import table as pose_table
from test_gpu_skin_vertices import small_case
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, frame, oracle_frame, same, scene
from test_morph_cpu import deltas_of
from test_normals_cpu import MESHES, indices_of, mesh_scene, ranges, rest_of, twisted
from test_skin_cpu import palette_of
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPLOADS = ("host", "device", "lbvh")


def upload(t, name, path="host"):
    if path == "host":
        t.upload_scene(mesh_scene(name).view)
    elif path == "device":
        t.upload_scene_device(mesh_scene(name, analytic_leaves_only=True).view, DEVICE_TREE)
    else:
        t.upload_scene_lbvh(mesh_scene(name).leaves_view())


def differences(got, want):
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    return f"{len(bad)} vertices differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}" if len(bad) else ""


def oracle_of(name, v, spp, integrator):
    """the oracle's frame of the host tree refitted around vertices v"""
    if name != "fan":
        return oracle_moved(name, v, spp, integrator)
    sc = mesh_scene(name)
    m = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, indices_of(name)), v)
    return oracle_frame(m.view, spp, integrator)


def status_of(call):
    with pytest.raises(TracerError) as e:
        call()
    return e.value.status


# --------------------------------------------------------------------------------------------------- vertices
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("name", MESHES)
def test_normals_are_the_definition_s(gpu, name, which):
    first, count = ranges(name)[which]
    v, idx = twisted(name), indices_of(name)
    upload(gpu, name)
    gpu.update_vertices(v)
    gpu.recompute_normals(first, count)
    got, want = gpu.download_vertices(), nr.recompute(v, idx, first, count)
    assert not differences(got, want)
    m = nr.in_range(len(v), first, count)
    assert np.array_equal(bits(got[:, :3]), bits(v[:, :3])) and np.array_equal(bits(got[:, 6:]), bits(v[:, 6:]))      # positions, uv
    assert np.array_equal(bits(got[~m]), bits(v[~m]))                                                                 # outside the range
    keep = np.isin(np.arange(len(v)), nr.kept(v, idx))
    assert (bits(got[m & ~keep, 3:6]) != bits(v[m & ~keep, 3:6])).any(axis=1).all() and (m & ~keep).sum() > 20
    assert which == 0 or (m & keep).sum() >= 2                           # the poles, the fan's planted vertices: in the whole range
    gpu.recompute_normals(first, count)                                  # a second call finds its own normals: the same bits
    assert not differences(gpu.download_vertices(), want)
    if which == 1:
        gpu.recompute_normals()                                          # the defaults are the whole mesh
        assert not differences(gpu.download_vertices(), want)


@pytest.mark.parametrize("path", UPLOADS)
@pytest.mark.parametrize("name", MESHES)
def test_every_upload_path_and_no_box_moves(gpu, name, path):
    first, count = ranges(name)[0]
    v, idx = twisted(name), indices_of(name)
    upload(gpu, name, path)
    gpu.update_vertices(v)
    tree = None if path == "host" else rr.raw(gpu.download_bvh())
    cost = bytes(gpu.tree_cost())
    gpu.recompute_normals(first, count)
    assert not differences(gpu.download_vertices(), nr.recompute(v, idx, first, count))
    assert bytes(gpu.tree_cost()) == cost
    if tree is not None:
        assert np.array_equal(rr.raw(gpu.download_bvh()), tree)
    # the call before any refit of the scene (the refit's root box has never been written), and rays still find the mesh
    upload(gpu, name, path)
    gpu.recompute_normals()
    assert not differences(gpu.download_vertices(), nr.recompute(rest_of(name), idx))
    got = frame(gpu, 4, PATH)
    with Tracer(0) as fresh:
        upload(fresh, name, path)
        assert not same(frame(fresh, 4, PATH), got)
        fresh.update_vertices(gpu.download_vertices())
        assert same(frame(fresh, 4, PATH), got)


# --------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("integrator", [PATH, MIS], ids=["path", "mis"])
@pytest.mark.parametrize("name", MESHES)
def test_frame_after_the_call_is_the_update_s_and_the_oracle_s(gpu, name, integrator):
    v = twisted(name)
    upload(gpu, name)
    gpu.update_vertices(v)
    before = frame(gpu, 4, integrator)
    gpu.recompute_normals()
    got = frame(gpu, 4, integrator)
    now = gpu.download_vertices()
    assert not differences(now, nr.recompute(v, indices_of(name)))
    assert not same(got, before)
    with Tracer(0) as fresh:                                            # the same tree, and the host's own normals passed in
        upload(fresh, name)
        fresh.update_vertices(now)
        assert same(frame(fresh, 4, integrator), got)
    assert same(got, oracle_of(name, now, 4, integrator))


@pytest.mark.parametrize("path", ["device", "lbvh"])
def test_frame_on_a_device_built_tree(gpu, path):
    v = twisted("mem")
    upload(gpu, "mem", path)
    gpu.update_vertices(v)
    first, count = ranges("mem")[0]
    gpu.recompute_normals(first, count)
    got = frame(gpu, 4, MIS)
    with Tracer(0) as fresh:
        upload(fresh, "mem", path)
        fresh.update_vertices(gpu.download_vertices())
        assert same(frame(fresh, 4, MIS), got)


# --------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("name", ["lds", "mem"])
def test_after_a_fused_morph_and_skin(gpu, name):
    v0, idx = rest_of(name), indices_of(name)
    n = len(v0)
    (mf, mc), (sf, sc_) = layouts(n)["overlap"]
    d, w = deltas_of(mc, 3), mr.weights(3, "negative")
    b, sw = sr.binding(sc_, 3)
    palette = palette_of(name, 3)
    upload(gpu, name)
    gpu.morph_bind(d, first=mf)
    gpu.skin_bind(b, sw, first=sf)
    gpu.morph_vertices(w, palette)
    fused = gpu.download_vertices()
    assert not differences(fused, mr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette))
    gpu.recompute_normals()
    got = gpu.download_vertices()
    assert not differences(got, nr.recompute(fused, idx))
    keep = np.isin(np.arange(n), nr.kept(fused, idx))
    assert (bits(got[~keep, 3:6]) != bits(fused[~keep, 3:6])).any(axis=1).all() and keep.sum() <= 2
    # the rest copy was not written: zero weights and no bones restore the rest bits of the morph binding, normals included
    gpu.morph_vertices(mr.weights(3, "zero"))
    back = gpu.download_vertices()
    assert np.array_equal(bits(back[mf:mf + mc]), bits(v0[mf:mf + mc]))
    assert np.array_equal(bits(back[mf + mc:]), bits(got[mf + mc:])) and np.array_equal(bits(back[:mf]), bits(got[:mf]))
    gpu.morph_vertices(w, palette)                                      # ... and the next fused call starts from rest again
    assert not differences(gpu.download_vertices(), mr.morph_skin(v0, back, mf, d, w, sf, b, sw, palette))


# --------------------------------------------------------------------------------------------------- the adjacency's lifetime
def test_adjacency_lifetime(gpu):
    v, idx = twisted("mem"), indices_of("mem")
    upload(gpu, "mem", "lbvh")
    gpu.update_vertices(v)
    first, count = ranges("mem")[0]
    gpu.recompute_normals(first, count)                                 # builds the adjacency
    want = nr.recompute(v, idx, first, count)
    assert not differences(gpu.download_vertices(), want)
    gpu.rebuild_tree(abi.TREE_SAH)                                      # kept by a rebuild, a triangle-material upload and an update
    gpu.upload_triangle_materials(np.full(len(idx) // 3, 4, np.uint32))
    v2 = rr.twist(rest_of("mem"), -0.4, 0.8)
    gpu.update_vertices(v2)
    gpu.recompute_normals()
    want = nr.recompute(v2, idx)
    assert not differences(gpu.download_vertices(), want)
    gpu.recompute_normals()                                             # two calls in a row: the same bits
    assert not differences(gpu.download_vertices(), want)
    gpu.upload_triangle_materials(None)
    for other in ("fan", "lds", "mem"):                                 # another scene in the same context: another adjacency
        upload(gpu, other)
        gpu.update_vertices(twisted(other))
        gpu.recompute_normals()
        assert not differences(gpu.download_vertices(), nr.recompute(twisted(other), indices_of(other))), other


# --------------------------------------------------------------------------------------------------- what is dropped and what is kept
def test_gbuffer_shows_the_new_normals(gpu):
    v = twisted("lds")
    upload(gpu, "lds")
    gpu.update_vertices(v)
    frame(gpu, 2, PATH)
    gpu.denoise()
    before = gpu.download_gbuffer()
    gpu.recompute_normals()
    frame(gpu, 2, PATH)
    gpu.denoise()
    after = gpu.download_gbuffer()
    with Tracer(0) as fresh:
        upload(fresh, "lds")
        fresh.update_vertices(gpu.download_vertices())
        frame(fresh, 2, PATH)
        fresh.denoise()
        want = fresh.download_gbuffer()
    assert after.tobytes() == want.tobytes()
    assert after["normal"].tobytes() != before["normal"].tobytes() and after["depth"].tobytes() == before["depth"].tobytes()


def test_triangle_materials_survive(gpu):
    from test_gpu_triangle_materials import Relabelled
    sc = scene("mem")
    rel = Relabelled(sc.view)
    gpu.upload_scene(rel.view(sc.view))
    gpu.upload_triangle_materials(np.full(sc.view.n_index // 3, rel.k, np.uint32))
    gpu.update_vertices(twisted("mem"))
    gpu.recompute_normals()
    now = gpu.download_vertices()
    assert same(frame(gpu, 4, MIS), oracle_of("mem", now, 4, MIS))
    gpu.upload_triangle_materials(None)


@pytest.mark.parametrize("single", [0, 1], ids=["per_depth", "single_launch"])
def test_both_values_of_refit_single(single):
    v, idx = twisted("mem"), indices_of("mem")
    with Tracer(0) as t:
        t.debug_set("refit_single", single)
        upload(t, "mem", "device")
        t.recompute_normals()                                           # before the refit maps exist ...
        t.update_vertices(v)
        t.recompute_normals()                                           # ... and after
        assert not differences(t.download_vertices(), nr.recompute(v, idx))
        got = frame(t, 4, PATH)
        with Tracer(0) as fresh:
            upload(fresh, "mem", "device")
            fresh.update_vertices(t.download_vertices())
            assert same(frame(fresh, 4, PATH), got)


def test_mesh_lights_frame_is_a_fresh_context_s(gpu):
    n_tri = len(indices_of("lds")) // 3
    tri_mat = np.full(n_tri, 4, np.uint32); tri_mat[n_tri // 2:n_tri // 2 + 6] = 3      # Cornell's table: 3 = the lamp's emitter, 4 = the red Lambert
    upload(gpu, "lds")
    gpu.upload_triangle_materials(tri_mat)
    gpu.update_vertices(twisted("lds"))
    before = frame(gpu, 4, MIS, mesh_lights=True)                       # the tables exist
    gpu.recompute_normals()
    got = frame(gpu, 4, MIS, mesh_lights=True)
    assert not same(got, before)
    with Tracer(0) as fresh:
        upload(fresh, "lds")
        fresh.upload_triangle_materials(tri_mat)
        fresh.update_vertices(gpu.download_vertices())
        assert same(frame(fresh, 4, MIS, mesh_lights=True), got)
    gpu.upload_triangle_materials(None)


def test_refit_ms_reports_the_family_s_last_call(gpu):
    upload(gpu, "mem")
    gpu.update_vertices(twisted("mem"))
    gpu.recompute_normals()
    a = gpu.refit_ms()
    assert 0.0 < a < 1000.0 and gpu.refit_ms() == a
    gpu.update_vertices(twisted("mem"))
    assert gpu.refit_ms() > a                                           # the same record rewrite and a launch per depth of the tree behind it


def test_refit_ms_is_every_call_s_own_whatever_came_before(gpu):
    """update, normals, pose, normals, skin, normals on one context: every call of the family is timed, the time is read once and then
    kept (a second read and a read behind a render return it again), and no call's bookkeeping disturbs another's vertices."""
    idx, poses = indices_of("mem"), pose_table("mem", "ragged")
    first, b, w, palette = small_case("mem")
    upload(gpu, "mem")
    state = {"now": rest_of("mem"), "rest": None}                       # the vertices as they stand; the rest copy (made by the first pose)

    def update():
        gpu.update_vertices(twisted("mem"))
        return twisted("mem")

    def normals():
        gpu.recompute_normals()
        return nr.recompute(state["now"], idx)

    def pose():
        state["rest"] = state["now"]
        gpu.pose_vertices(poses)
        return pr.pose(state["rest"], state["now"], poses)

    def skin():
        gpu.skin_bind(b, w, first=first)
        gpu.skin_vertices(palette)
        return sr.skin(state["rest"], state["now"], first, b, w, palette)

    for step, call in enumerate((update, normals, pose, normals, skin, normals)):
        state["now"] = call()
        ms = gpu.refit_ms()
        assert 0.0 < ms < 1000.0, (step, ms)
        assert gpu.refit_ms() == ms, step
        frame(gpu, 1, PATH)
        assert gpu.refit_ms() == ms, step
        assert not differences(gpu.download_vertices(), state["now"]), step
        if call is not normals:
            assert gpu.pose_overflows() == 0, step


# --------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        assert status_of(lambda: fresh.recompute_normals(0, 1)) == abi.ERR_NO_SCENE
        assert status_of(lambda: fresh.recompute_normals(0, 0)) == abi.ERR_NO_SCENE
        spheres = host.HostScene(abi.SCENE_CORNELL_SPHERES)                        # a scene without triangles; kept alive: its view
        fresh.upload_scene(spheres.view)                                           # points into memory the scene owns
        fresh.recompute_normals(0, 0)                                              # count == 0: TRC_OK
        fresh.recompute_normals(7, 0)
        assert status_of(lambda: fresh.recompute_normals(0, 1)) == abi.ERR_INVALID_ARG
    v = twisted("lds")
    n = len(v)
    upload(gpu, "lds")
    gpu.update_vertices(v)
    before = frame(gpu, 4, MIS)
    gpu.denoise()
    gbuffer = gpu.download_gbuffer()

    def unchanged():
        assert np.array_equal(bits(gpu.download_vertices()), bits(v))
        assert gpu.download_gbuffer().tobytes() == gbuffer.tobytes()
        assert same(frame(gpu, 4, MIS), before)
        gpu.denoise()
        assert gpu.download_gbuffer().tobytes() == gbuffer.tobytes()

    for first, count in ((0, n + 1), (1, n), (n, 1), (n - 1, 2), (0xFFFFFFFF, 1), (2, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert not nr.valid_range(first, count, n)
        assert status_of(lambda: gpu.recompute_normals(first, count)) == abi.ERR_INVALID_ARG, (first, count)
        unchanged()
    for first in (0, 5, n, n + 1, 0xFFFFFFFF):                                     # count == 0: TRC_OK, nothing happens, nothing is dropped
        gpu.recompute_normals(first, 0)
        unchanged()
    gpu.recompute_normals(n - 1, 1)                                                # up to the last vertex: accepted (a pole: it keeps its bits)
    assert np.array_equal(bits(gpu.download_vertices()), bits(v))


# --------------------------------------------------------------------------------------------------- the example host
def test_example_host_normals(tmp_path):
    """examples/trc_render --morph 2 --normals on a skew pyramid, through the C ABI only: the normals change the frames.  (Not the
    tetrahedron of the other example tests: pressed to half its height, three of its four smooth normals stay on their axes.)"""
    obj, out = tmp_path / "pyramid.obj", tmp_path / "f.png"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 1 0 1\nv 0 0 1\nv 0.3 1 0.4\nf 1 2 3\nf 1 3 4\nf 1 5 2\nf 2 5 3\nf 3 5 4\nf 4 5 1\n")
    exe = [os.path.join(ROOT, "examples", "trc_render"), "--mesh", str(obj), "--size", "48", "32", "--spp", "8", "--out", str(out)]
    r = subprocess.run(exe + ["--morph", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "trc_recompute_normals" not in r.stdout
    plain = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (1, 2)]
    r = subprocess.run(exe + ["--morph", "2", "--normals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("trc_recompute_normals, first call") == 1 and r.stdout.count("ms, trc_recompute_normals") == 2
    smooth = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (1, 2)]
    assert smooth[0].shape == plain[0].shape
    assert not np.array_equal(smooth[0], plain[0])      # frame 1 is pressed to half its height; frame 2 is the rest shape again, whose normals the loader made the same way
