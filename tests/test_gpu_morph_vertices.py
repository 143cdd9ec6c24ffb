"""trc_morph_bind / trc_morph_vertices on the GPU (include/tracer_abi.h): the morphed vertices against the definition
(tests/morph_ref.py) bit for bit, alone and with the skin of trc_skin_bind on top in the same call, and everything behind them -- tree,
frames, what is kept and what is dropped -- against what trc_update_vertices leaves for the same vertices, against the definition of
the refit (tests/refit_ref.py) and against the CPU oracle.  The bindings (tests/test_skin_cpu.py) put a lane, a wavefront and a
256-thread boundary inside the bound range, with both of its ends unaligned; the target counts (tests/test_morph_cpu.py) lie on both
sides of the kernel's unroll factor; three rest vertices hold a -0, set through trc_update_vertices."""
import os
import subprocess

import numpy as np
import pytest

import morph_ref as mr
import pose_ref as pr
import refit_ref as rr
import skin_ref as sr
from test_gpu_pose_vertices import bits, matrices, oracle_moved, overflows
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, first_difference, frame, same, scene
from test_morph_cpu import PLANTED, TARGETS, deltas_of, planted_rest
from test_skin_cpu import bindings, palette_of
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plant(t, residence):
    """the -0 of test_morph_cpu.PLANTED into the uploaded scene, as a caller would: trc_update_vertices; -> the rest vertices"""
    v0 = planted_rest(residence)
    lo, hi = min(PLANTED[residence]), max(PLANTED[residence]) + 1
    t.update_vertices(v0[lo:hi], first=lo)
    return v0


def upload(t, residence):
    t.upload_scene(scene(residence).view)
    return plant(t, residence)


def small_case(residence, which=0, n_targets=3, kind="negative"):
    """(first, deltas, weights) of the residence's first (ragged) or second (whole) binding"""
    first, count = bindings(residence)[which]
    return first, deltas_of(count, n_targets), mr.weights(n_targets, kind)


def status_of(call):
    with pytest.raises(TracerError) as e:
        call()
    return e.value.status


def layouts(n):
    """name -> ((morph first, count), (skin first, count)) on n vertices"""
    third = n // 3
    return {"identical": ((2, n - 5), (2, n - 5)),
            "overlap": ((2, n // 2), (third, n - third - 1)),            # morph only | both | skin only; the last vertex in neither
            "apart": ((1, third), (third + 3, n - third - 4))}          # two vertices of the hull between them, in neither


# --------------------------------------------------------------------------------------------------- vertices
@pytest.mark.parametrize("kind", mr.WEIGHT_KINDS)
@pytest.mark.parametrize("n_targets", TARGETS)
@pytest.mark.parametrize("which", [0, 1], ids=["ragged", "whole"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_morphed_vertices_are_the_definition_s(gpu, residence, which, n_targets, kind):
    first, d, w = small_case(residence, which, n_targets, kind)
    count = d.shape[1]
    v0 = upload(gpu, residence)
    assert mr.valid_binding(first, d, len(v0)) and mr.valid_weights(w, n_targets)
    gpu.morph_bind(d, first=first)
    assert np.array_equal(bits(gpu.download_vertices()), bits(v0))                       # a bind alone moves no vertex
    gpu.morph_vertices(w)
    got, want = gpu.download_vertices(), mr.morph(v0, v0, first, d, w)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} vertices differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    m = np.zeros(len(v0), bool)
    m[first:first + count] = True
    assert np.array_equal(bits(got[~m]), bits(v0[~m]))
    assert (bits(got[m]) != bits(v0[m])).any(axis=1).all() if mr.active(w) else np.array_equal(bits(got), bits(v0))
    assert gpu.pose_overflows() == 0
    gpu.morph_vertices(mr.weights(n_targets, "zero"))                                    # all-zero weights undo it: the rest bits, -0 included
    assert np.array_equal(bits(gpu.download_vertices()), bits(v0))
    assert np.signbit(v0[list(PLANTED[residence]), 3]).all()


def test_overflow_is_counted_and_zero_weights_restore(gpu):
    """The count is the definition's: final positions that are not finite or beyond 1e37.  A delta of 3e30 under a weight of 1e6 leaves
    every position near 3e36, inside the bound (count 0); under 1e8 the product is 3e38 and all nine bound vertices are past it.  Nothing
    is rendered between an overflow and the morph that undoes it."""
    v0 = upload(gpu, "lds")
    d = np.zeros((1, 9, 6), F)
    d[0, :, 0] = F(3e30)
    gpu.morph_bind(d, first=2)
    assert gpu.pose_overflows() == 0
    for weight in (1e6, 1e8):
        gpu.morph_vertices([weight])
        with np.errstate(all="ignore"):
            want = overflows(mr.morph(v0, v0, 2, d, [weight])[2:11, :3])
        assert gpu.pose_overflows() == want, weight
    assert want == 9
    gpu.morph_vertices([0.0])
    assert gpu.pose_overflows() == 0
    got = gpu.download_vertices()
    assert np.array_equal(bits(got), bits(v0))
    assert same(frame(gpu, 4, PATH), oracle_moved("lds", got, 4, PATH))


# --------------------------------------------------------------------------------------------------- the skin on top
@pytest.mark.parametrize("n_bones", [3, abi.SKIN_LDS_BONES + 1])
@pytest.mark.parametrize("layout", ["identical", "overlap", "apart"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_fused_call_is_the_skin_of_the_morphed_vertices(gpu, residence, layout, n_bones):
    v0 = upload(gpu, residence)
    n = len(v0)
    (mf, mc), (sf, sc_) = layouts(n)[layout]
    d, w = deltas_of(mc, 3), mr.weights(3, "negative")
    b, sw = sr.binding(sc_, n_bones)
    palette = palette_of(residence, n_bones)
    everywhere = [(0, n, *matrices(residence, "A"))]
    gpu.pose_vertices(everywhere)                                       # so that a vertex that is not written shows: no vertex is at rest
    posed = pr.pose(v0, v0, everywhere)
    assert (bits(posed) != bits(v0)).any(axis=1).all()
    gpu.morph_bind(d, first=mf)
    gpu.skin_bind(b, sw, first=sf)
    gpu.morph_vertices(w, palette)
    got, want = gpu.download_vertices(), mr.morph_skin(v0, posed, mf, d, w, sf, b, sw, palette)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} vertices differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    assert gpu.pose_overflows() == 0
    # the kinds of vertex, each from its own definition
    i = np.arange(n)
    in_m, in_s = (i >= mf) & (i < mf + mc), (i >= sf) & (i < sf + sc_)
    morphed = mr.morph(v0, v0, mf, d, w)
    assert np.array_equal(bits(got[in_m & ~in_s]), bits(morphed[in_m & ~in_s]))
    assert np.array_equal(bits(got[in_s & ~in_m]), bits(sr.skin(v0, v0, sf, b, sw, palette)[in_s & ~in_m]))
    assert np.array_equal(bits(got[in_s & in_m]), bits(sr.skin(morphed, morphed, sf, b, sw, palette)[in_s & in_m]))
    assert np.array_equal(bits(got[~in_s & ~in_m]), bits(posed[~in_s & ~in_m]))
    hull = (i >= min(mf, sf)) & (i < max(mf + mc, sf + sc_))
    if layout == "identical":
        assert (in_m == in_s).all()
    elif layout == "overlap":
        assert (in_m & ~in_s).any() and (in_s & ~in_m).any() and (in_m & in_s).any() and not (hull & ~in_m & ~in_s).any()
        assert not np.array_equal(bits(got[in_s & in_m]), bits(sr.skin(v0, v0, sf, b, sw, palette)[in_s & in_m]))      # not the skin of rest
    else:
        assert (hull & ~in_m & ~in_s).sum() == 2 and not (in_m & in_s).any()
    # every weight zero: trc_skin_vertices bit for bit, and the morph-only vertices at rest
    gpu.morph_vertices(mr.weights(3, "zero"), palette)
    zeroed = gpu.download_vertices()
    gpu.skin_vertices(palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(zeroed))
    assert np.array_equal(bits(zeroed[in_s]), bits(sr.skin(v0, v0, sf, b, sw, palette)[in_s]))
    assert np.array_equal(bits(zeroed[in_m & ~in_s]), bits(v0[in_m & ~in_s]))
    # a plain skin after a fused call skins from rest
    gpu.morph_vertices(w, palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))
    gpu.skin_vertices(palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(sr.skin(v0, want, sf, b, sw, palette)))


# --------------------------------------------------------------------------------------------------- tree
@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


@pytest.mark.parametrize("tree", ["sah_triangle_leaves", "lbvh"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_downloaded_tree_is_the_refit_of_the_tree_before(tracer, residence, tree):
    """a morph, a fused call and a morph again, so that a counter the single launch did not put back shows in a later result"""
    sc = scene(residence)
    if tree == "lbvh":
        tracer.upload_scene_lbvh(sc.leaves_view())
    else:
        tracer.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    before = rr.raw(tracer.download_bvh())
    v0, idx = plant(tracer, residence), rr.indices_of(sc.view)
    (mf, mc), (sf, sc_) = layouts(len(v0))["overlap"]
    d = deltas_of(mc, 3)
    b, sw = sr.binding(sc_, 3)
    palette = palette_of(residence, 3)
    tracer.morph_bind(d, first=mf)
    tracer.skin_bind(b, sw, first=sf)
    current = v0
    for kind, bones in (("negative", None), ("all", palette), ("alternating", None)):
        w = mr.weights(3, kind)
        tracer.morph_vertices(w, bones)
        current = mr.morph(v0, current, mf, d, w) if bones is None else mr.morph_skin(v0, current, mf, d, w, sf, b, sw, palette)
        assert np.array_equal(bits(tracer.download_vertices()), bits(current)), kind
        got = rr.raw(tracer.download_bvh())
        assert not first_difference(got, rr.refit(before, current, idx)), kind
    assert (got[:, :8] == before[:, :8]).all()                       # links, axis, pType, pIndex: the topology stays


# --------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_frame_after_morph_is_the_update_s_and_the_oracle_s(gpu, residence):
    sc = scene(residence)
    v0 = upload(gpu, residence)
    first, d, w = small_case(residence)
    v = mr.morph(v0, v0, first, d, w)
    original = frame(gpu, 4, MIS)
    gpu.morph_bind(d, first=first)
    gpu.morph_vertices(w)
    got = frame(gpu, 4, MIS)
    assert not same(got, original)
    assert same(got, oracle_moved(residence, v, 4, MIS))
    with Tracer(0) as fresh:                                            # ... and what the host's own arithmetic, passed in, gives
        fresh.upload_scene(sc.view)
        fresh.update_vertices(v)
        assert same(frame(fresh, 4, MIS), got)


def test_frame_after_a_fused_call_is_the_update_s(gpu):
    sc = scene("mem")
    v0 = upload(gpu, "mem")
    (mf, mc), (sf, sc_) = layouts(len(v0))["overlap"]
    d, w = deltas_of(mc, 3), mr.weights(3, "negative")
    b, sw = sr.binding(sc_, 3)
    palette = palette_of("mem", 3)
    gpu.morph_bind(d, first=mf)
    gpu.skin_bind(b, sw, first=sf)
    gpu.morph_vertices(w, palette)
    got = frame(gpu, 4, MIS)
    v = mr.morph_skin(v0, v0, mf, d, w, sf, b, sw, palette)
    with Tracer(0) as fresh:
        fresh.upload_scene(sc.view)
        fresh.update_vertices(v)
        assert same(frame(fresh, 4, MIS), got)


# --------------------------------------------------------------------------------------------------- the binding's lifetime
def test_binding_lifetime(gpu):
    sc = scene("lds")
    gpu.upload_scene_lbvh(sc.leaves_view())
    v0 = plant(gpu, "lds")
    first, d, w = small_case("lds")
    gpu.morph_bind(d, first=first)
    gpu.morph_vertices(w)
    want = mr.morph(v0, v0, first, d, w)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))
    # a rebind replaces the binding: the old range keeps its morphed values, the new one is computed from rest
    d2, w2 = mr.deltas(2, 4, seed=21), mr.weights(2, "all")
    gpu.morph_bind(d2, first=1)
    gpu.morph_vertices(w2)
    want = mr.morph(v0, want, 1, d2, w2)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want))
    # trc_rebuild_tree, update_vertices, pose_vertices, skin_bind / skin_vertices and upload_triangle_materials keep it
    gpu.rebuild_tree(abi.TREE_SAH)
    rest = v0.copy()
    rest[2:4] = rr.twist(v0, 0.3, 0.9)[2:4]
    gpu.update_vertices(rest[2:4], first=2)
    gpu.pose_vertices([(0, 3, *matrices("lds", "B"))])
    b, sw = sr.binding(3, 3)
    gpu.skin_bind(b, sw, first=6)
    gpu.skin_vertices(palette_of("lds", 3))
    gpu.upload_triangle_materials(np.full(sc.view.n_index // 3, 4, np.uint32))
    current = gpu.download_vertices()
    gpu.morph_vertices(w2)
    got = gpu.download_vertices()
    assert np.array_equal(bits(got), bits(mr.morph(rest, current, 1, d2, w2)))
    assert not np.array_equal(bits(got[1:5]), bits(want[1:5]))                         # the update moved rest vertices of the range
    gpu.upload_triangle_materials(None)
    # an empty table unbinds, whichever of its two extents is zero
    for empty in (d2[:0], d2[:, :0]):
        gpu.morph_bind(d2, first=1)
        gpu.morph_bind(empty)
        assert status_of(lambda: gpu.morph_vertices(w2)) == abi.ERR_INVALID_ARG
    assert gpu._L.trc_morph_bind(gpu._h, None, 0, 0, 0) == abi.OK                       # deltas may be NULL with an empty table
    assert np.array_equal(bits(gpu.download_vertices()), bits(got))
    # an upload drops the binding
    gpu.morph_bind(d2, first=1)
    gpu.upload_scene(sc.view)
    assert status_of(lambda: gpu.morph_vertices(w2)) == abi.ERR_INVALID_ARG
    assert np.array_equal(bits(gpu.download_vertices()), bits(rr.vertices_of(sc.view)))


# --------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        d1 = mr.deltas(1, 1)
        assert status_of(lambda: fresh.morph_bind(d1)) == abi.ERR_NO_SCENE
        assert status_of(lambda: fresh.morph_vertices([1.0])) == abi.ERR_NO_SCENE
        spheres = host.HostScene(abi.SCENE_CORNELL_SPHERES)                        # a scene without triangles; kept alive: its view
        fresh.upload_scene(spheres.view)                                           # points into memory the scene owns
        fresh.morph_bind(d1[:0])                                                   # an empty table: TRC_OK
        assert status_of(lambda: fresh.morph_bind(d1)) == abi.ERR_INVALID_ARG
        assert status_of(lambda: fresh.morph_vertices([1.0])) == abi.ERR_INVALID_ARG
    v0 = upload(gpu, "lds")
    n = len(v0)
    first, d, w = small_case("lds")
    count = d.shape[1]
    b, sw = sr.binding(count, 3)
    palette = palette_of("lds", 3)
    gpu.morph_bind(d, first=first)
    gpu.morph_vertices(w)                                                         # refusals on a context that has morphed once
    verts, before = gpu.download_vertices(), frame(gpu, 4, MIS)

    def unchanged():
        assert np.array_equal(bits(gpu.download_vertices()), bits(verts))
        assert same(frame(gpu, 4, MIS), before)

    # ---- trc_morph_bind
    refused = [(first + 6, d), (n, d[:, :1]), (0xFFFFFFFF, d[:, :2])]
    for c, bad in ((0, np.nan), (2, np.inf), (3, -np.inf), (5, np.nan)):
        d_bad = d.copy(); d_bad[2, count - 1, c] = bad
        refused.append((first, d_bad))
    refused.append((0, np.zeros((abi.TRC_MORPH_MAX_TARGETS + 1, 1, 6), F)))
    for f, dd in refused:
        assert not mr.valid_binding(f, dd, n)
        assert status_of(lambda: gpu.morph_bind(dd, first=f)) == abi.ERR_INVALID_ARG, (f, dd.shape)
        unchanged()
    table = np.zeros((2, 4, 6), F)
    assert gpu._L.trc_morph_bind(gpu._h, None, 2, 0, 2) == abi.ERR_INVALID_ARG                        # NULL with a non-empty table
    assert gpu._L.trc_morph_bind(gpu._h, table.ctypes.data, 2, 2, 0xFFFFFFFF) == abi.ERR_INVALID_ARG  # first + count wraps
    assert gpu._L.trc_morph_bind(gpu._h, table.ctypes.data, 0xFFFFFFFF, 0, 4) == abi.ERR_INVALID_ARG  # refused before a delta is read
    unchanged()
    gpu.morph_vertices(w)                                                         # a refused rebind leaves the old binding working
    unchanged()
    # ---- trc_morph_vertices
    for ww in (w[:2], np.append(w, F(1)), [w[0], np.nan, w[2]], [np.inf, w[1], w[2]], [w[0], w[1], -np.inf]):
        assert not mr.valid_weights(ww, 3)
        assert status_of(lambda: gpu.morph_vertices(ww)) == abi.ERR_INVALID_ARG
        unchanged()
    assert gpu._L.trc_morph_vertices(gpu._h, None, 3, None, 0) == abi.ERR_INVALID_ARG                 # weights == NULL
    unchanged()
    assert status_of(lambda: gpu.morph_vertices(w, palette)) == abi.ERR_INVALID_ARG                    # bones without a skin binding
    unchanged()
    gpu.skin_bind(b, sw, first=first)
    nan = palette[1][0].copy(); nan[2, 3] = np.nan
    for pal in (palette[:2], [palette[0], (nan, palette[1][1]), palette[2]]):                          # what trc_skin_vertices refuses
        assert not sr.valid_palette(pal, b.max())
        assert status_of(lambda: gpu.morph_vertices(w, pal)) == abi.ERR_INVALID_ARG
        unchanged()
    w_buf = np.ascontiguousarray(w)
    assert gpu._L.trc_morph_vertices(gpu._h, w_buf.ctypes.data, 3, None, 3) == abi.ERR_INVALID_ARG    # bones == NULL with n_bones > 0
    unchanged()
    gpu.morph_vertices(w)                                                         # n_bones == 0: morph only, whatever the skin binding
    unchanged()
    gpu.morph_bind(d[:0])
    assert status_of(lambda: gpu.morph_vertices(w)) == abi.ERR_INVALID_ARG       # no binding
    unchanged()


# --------------------------------------------------------------------------------------------------- the example host
def test_example_host_morph(tmp_path):
    """examples/trc_render --morph 2 on a tetrahedron, alone and after --bend 1 (the fused call), through the C ABI only"""
    obj, out = tmp_path / "tet.obj", tmp_path / "f.png"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 3 2\nf 1 2 4\nf 2 3 4\nf 1 4 3\n")
    exe = [os.path.join(ROOT, "examples", "trc_render"), "--mesh", str(obj), "--size", "48", "32", "--spp", "2", "--out", str(out)]
    r = subprocess.run(exe + ["--morph", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("trc_morph_vertices") == 2 and "under two bones" not in r.stdout
    frames = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (1, 2)]
    assert frames[0].shape == frames[1].shape == host.load_png(out).shape
    assert not np.array_equal(frames[0], frames[1])
    r = subprocess.run(exe + ["--bend", "1", "--morph", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("trc_skin_vertices") == 1 and r.stdout.count("trc_morph_vertices under two bones") == 2
    fused = [host.load_png(tmp_path / f"f.png.{k}.png") for k in (2, 3)]
    assert not np.array_equal(fused[0], frames[0])                                 # half a turn of the top on the same morph
