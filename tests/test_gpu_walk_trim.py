"""The two short forms of dev_intersect.hpp, bit for bit against the oracle's literal walk:

  * square_hit_test builds the record of an accepted square from selects -- +-1 at axis_k and two zeros that carry the
    SIGN of the flip (Square.hh:98-108 + HitRecord.hh:26-29 give -0 where the face is flipped), value_k / a / b at their axes;
  * box_hit / box_hit_t drop `|| tmax < 0` and `tmin < 0 ? tmax : tmin` (AABB.hh:86,106,110), valid because range_t.x is FLT_MIN.

Through the Scene::hit hook (trc_trace_rays: the whole HitRecord per ray, compared as uint32) on the hooks build, instrumented
walk (counters included: every box decision) and TRC_TRACE_PRODUCTION, on a hand-made scene of six squares -- the faces of
the cube [-10, 10]^3, one per orientation and side, each seen from inside and from outside, with gaps along most edges so
that a ray from anywhere can meet any of them first -- and one small frame of the path kernel.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_rays
from oracle import pyoracle as po
from tracer_amd import abi, host
from test_gpu_traversal import HIT_FIELDS, _materials, _square, assert_records_equal

F32 = np.float32
FLT_MIN = float(np.finfo(F32).tiny)
COUNTERS = ["n_descend", "n_return", "n_leaf"]
PAD = 1.0 / 512                  # _square pads the thin axis of a square's box by this much (exact in binary32)


def six_squares():
    """-> (scene view, keep-alive).  Square 2 * axis + side is the face `axis = -10 / +10`.  The faces span [-8, 8] on their two
    axes, except that the x = -10 wall and the floor (y = -10) reach down / left to -10.  The boxes are one unit wider than the
    squares in their planes -- an axis-parallel ray exactly on a box face misses the box (0 * inf), and the batch wants such rays
    exactly on the squares' range bounds -- except the floor's, which starts at x = -10: exactly where a ray travelling along +x
    has just hit the x = -10 wall."""
    mats = _materials()
    squares, leaves = [], []
    for ak in range(3):
        for side, k in enumerate((-10.0, 10.0)):
            lo_i = lo_j = -8.0
            if (ak, side) == (0, 0): lo_i = -10.0        # x = -10 wall: y from -10 (axis_i of an x square is y)
            if (ak, side) == (1, 0): lo_i = -10.0        # floor: x from -10 (axis_i of a y square is x)
            q, lo, hi = _square(ak, lo_i, 8.0, lo_j, 8.0, k, 2 * ak + side)
            for axis in (q.axis_i, q.axis_j):
                if (ak, side, axis) != (1, 0, 0): lo[axis] -= 1.0
                hi[axis] += 1.0
            squares.append(q)
            leaves.append(host.build_node(lo, hi, abi.PRIM_SQUARE, len(squares) - 1))
    nodes = host.build_tree(leaves)
    sarr = (abi.Square * len(squares))(*squares)
    marr = (abi.Material * len(mats))(*mats)
    sv = abi.Scene()
    sv.bvhList, sv.n_bvh = C.cast(nodes, C.POINTER(abi.BVH)), len(nodes)
    sv.squareList, sv.n_square = C.cast(sarr, C.POINTER(abi.Square)), len(squares)
    sv.materials, sv.n_material = C.cast(marr, C.POINTER(abi.Material)), len(mats)
    return sv, [nodes, sarr, marr]


def seeded_rays(n=6000, seed=2101):
    rs = np.random.RandomState(seed)
    o = np.concatenate([rs.uniform(-9.5, 9.5, (n // 2, 3)), rs.uniform(-30, 30, (n - n // 2, 3))]).astype(F32)
    d = rs.normal(size=(n, 3)).astype(F32)
    return make_rays(o, d)


def adversarial_rays():
    """-> (rays, {class name: ray indices}, the axis of each "own axis" ray).  Every ray is written down; the kernel normalises
    the direction (a zero stays a zero of its sign)."""
    o, d, tm, where, own_axis = [], [], [], {}, []
    big = float(np.finfo(F32).max)

    def add(name, origin, direction, tmax=big):
        where.setdefault(name, []).append(len(o))
        o.append(origin); d.append(direction); tm.append(tmax)

    zeros = (0.0, -0.0)
    for ak in range(3):
        ai, aj = [(1, 2), (0, 2), (0, 1)][ak]
        for sgn in (1.0, -1.0):
            for zi in zeros:
                for zj in zeros:
                    dirv = [0.0] * 3; dirv[ak], dirv[ai], dirv[aj] = sgn, zi, zj
                    for start in (0.0, -25.0 * sgn):             # from inside the cube, and from outside through both faces
                        org = [0.5, -0.25, 0.75]; org[ak] = start
                        add("axis-parallel, +0 / -0 on the two other axes", org, dirv)
                        # ... exactly ON the range_i / range_j bounds (a = o_i + t * +-0 = o_i), and one ulp outside
                        for bi in (-8.0, 8.0, float(np.nextafter(F32(8), F32(9))), float(np.nextafter(F32(-8), F32(-9)))):
                            for bj in (-8.0, 8.0, 0.5):
                                org = [0.0] * 3; org[ak], org[ai], org[aj] = start, bi, bj
                                add("hits on the range bounds", org, dirv)
                                org = [0.0] * 3; org[ak], org[ai], org[aj] = start, bj, bi
                                add("hits on the range bounds", org, dirv)
        # the square's OWN axis is +0 / -0: t = +-inf off its plane, NaN on it -- rejected, while the other faces are still hit
        for zk in zeros:
            for on_plane in (False, True):
                for slope in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-0.3, 0.1)):
                    dirv = [0.0] * 3; dirv[ak], dirv[ai], dirv[aj] = zk, slope[0], slope[1]
                    org = [1.5, -2.5, 3.5]; org[ak] = 10.0 if on_plane else 4.0
                    add("own axis +0 / -0", org, dirv)
                    org = list(org); org[ak] = -10.0 if on_plane else -25.0       # outside the cube: misses everything, or skims a plane
                    add("own axis +0 / -0", org, dirv)
                    own_axis += [ak, ak]
        # origins ON a square's plane, leaving it either way (t = +-0 < range_t.x: that square is rejected) or obliquely
        for k in (-10.0, 10.0):
            for dk in (1.0, -1.0, 0.25, -0.25):
                for tilt in (0.0, -0.0, 0.5):
                    dirv = [0.0] * 3; dirv[ak], dirv[ai], dirv[aj] = dk, tilt, -tilt
                    org = [1.0, 2.0, -3.0]; org[ak] = k
                    add("origin on a plane", org, dirv)
        # a node box entered exactly at t == range_t.y: tmax = the distance to the near face of a square's (padded) box, to the
        # plane itself (Square::hit_test accepts t == range_t.y), one ulp either side of both
        for sgn in (1.0, -1.0):
            dirv = [0.0] * 3; dirv[ak] = sgn
            org = [0.5, -0.25, 0.75]; org[ak] = -26.0 * sgn
            for dist in (16.0 - PAD, 16.0, 16.0 + PAD, 36.0 - PAD, 36.0):
                for t in (np.nextafter(F32(dist), F32(0)), F32(dist), np.nextafter(F32(dist), F32(100))):
                    add("box entered at t == range_t.y", org, dirv, float(t))
            org = list(org); org[ak] = 0.0
            for dist in (10.0 - PAD, 10.0, 10.0 + PAD):
                for t in (np.nextafter(F32(dist), F32(0)), F32(dist), np.nextafter(F32(dist), F32(100))):
                    add("box entered at t == range_t.y", org, dirv, float(t))
    # ... and with range_t.y lowered by the walk itself: along +x just above the floor's plane, inside the floor's box: the x = -10
    # wall is hit at t = 10, and the floor's box (x from -10) is entered at exactly that t
    for y in (-10.0 + PAD / 2, -10.0 - PAD / 2, -10.0 + PAD, -10.0):
        for z in (0.0, -8.0, 8.0):
            for zy in zeros:
                add("box entered at t == range_t.y", [-20.0, y, z], [1.0, zy, 0.0])
                add("box entered at t == range_t.y", [-20.0, y, z], [1.0, zy, -0.0], 10.0)
    # tmax negative, zero of either sign, denormal (below FLT_MIN = range_t.x), FLT_MIN itself and just above it: from inside
    # every box, from inside the root box only, from outside, on a plane
    for tmax in (-1.0, -big, -0.0, 0.0, -1e-40, 1e-45, 1e-40, float(np.nextafter(F32(FLT_MIN), F32(0))), FLT_MIN,
                 float(np.nextafter(F32(FLT_MIN), F32(1))), 3 * FLT_MIN):
        for org in ([0.5, -0.25, 0.75], [10.0, 1.0, 1.0], [10.0 + PAD, 1.0, 1.0], [-25.0, 0.0, 0.0], [-10.0, -10.0, -10.0]):
            for dirv in ([1.0, 0.0, 0.0], [-1.0, -0.0, 0.0], [0.3, -0.5, 0.8], [0.0, 0.0, -1.0]):
                add("tmax negative / denormal", org, dirv, tmax)
    rays = make_rays(np.array(o, F32), np.array(d, F32), np.array(tm, F32))
    return rays, {k: np.array(v) for k, v in where.items()}, np.array(own_axis)


@pytest.fixture(scope="module")
def six(gpu_hooks):
    sv, keep = six_squares()
    gpu_hooks.upload_scene(sv)
    return sv, keep


def _held_to_the_oracle(gpu_hooks, sv, rays, what):
    ref = po.trace_rays(sv, rays)
    assert_records_equal(gpu_hooks.trace_rays(rays), ref, HIT_FIELDS + COUNTERS, what=what + ", instrumented")
    assert_records_equal(gpu_hooks.trace_rays(rays, production=True), ref, what=what + ", production")
    return ref


@pytest.mark.gpu
def test_seeded_rays_on_six_squares(gpu_hooks, six):
    sv, _ = six
    ref = _held_to_the_oracle(gpu_hooks, sv, seeded_rays(), "seeded")
    hit = ref["hit"] != 0
    assert set(np.unique(ref["pIndex"][hit])) == set(range(6))               # every face is somebody's closest hit ...
    for idx in range(6):                                                     # ... from its kept and from its flipped side
        n_k = ref["sn"][hit & (ref["pIndex"] == idx)][:, idx // 2]
        assert (n_k == 1).any() and (n_k == -1).any()
    # the flipped record carries NEGATIVE zeros (HitRecord.hh:28: sn = -gn), the kept one positive ones
    sn = ref["sn"][hit].view(np.uint32)
    assert set(np.unique(sn)) == {0x00000000, 0x80000000, 0x3F800000, 0xBF800000}
    flipped = (sn == 0xBF800000).any(axis=1)
    assert ((sn[flipped] == 0x80000000).sum(axis=1) == 2).all() and ((sn[~flipped] == 0).sum(axis=1) == 2).all()


@pytest.mark.gpu
def test_adversarial_rays_on_six_squares(gpu_hooks, six):
    sv, _ = six
    rays, where, own_axis = adversarial_rays()
    ref = _held_to_the_oracle(gpu_hooks, sv, rays, "adversarial")
    hit = ref["hit"] != 0
    cls = lambda name: where[name]
    # the batch does what it is meant to
    assert hit[cls("axis-parallel, +0 / -0 on the two other axes")].all()
    on_bounds = hit[cls("hits on the range bounds")]
    assert 0.3 < on_bounds.mean() < 0.9                                      # the bounds themselves hit, one ulp outside passes through the gap
    own = cls("own axis +0 / -0")
    assert hit[own].any() and not hit[own].all()
    assert (ref["pIndex"][own][hit[own]] // 2 != own_axis[hit[own]]).all()   # never a square the ray is parallel to
    assert (ref["t"][cls("origin on a plane")][hit[cls("origin on a plane")]] > 1.0).all()      # the plane the ray starts on is rejected
    entered = hit[cls("box entered at t == range_t.y")]
    assert entered.any() and not entered.all()
    short = cls("tmax negative / denormal")
    assert not hit[short].any()
    assert ref["n_descend"][short].any() and not ref["n_descend"][short].all()   # some pass the root box (tmax >= FLT_MIN inside it), some do not
    # any-hit: the order-free production walk of shadow rays runs the same two box tests
    ref_any = po.trace_rays(sv, rays, any_hit=True)
    assert_records_equal(gpu_hooks.trace_rays(rays, any_hit=True, production=True), ref_any, ["hit"], what="adversarial any-hit, production")
    assert_records_equal(gpu_hooks.trace_rays(rays, any_hit=True), ref_any, HIT_FIELDS + COUNTERS, what="adversarial any-hit, instrumented")


@pytest.mark.gpu
def test_small_frame_of_the_path_kernel(gpu, cornell_spheres):
    W, H, spp, seed = 64, 64, 8, 2121
    cam = host.prepare_camera(W, H)
    gpu.upload_scene(cornell_spheres.view); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(seed); gpu.clear_accum(); gpu.reset_stats()
    gpu.render(spp=spp, integrator=abi.INTEGRATOR_PATH)
    dev, st = gpu.download_accum(), gpu.stats()
    ref, ref_st = po.render(cornell_spheres.view, cam, W, H, host.fill_rng(seed, W, H), spp=spp)
    assert st.rays == ref_st.rays and st.paths == W * H * spp
    assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32))


def test_the_batches_cover_what_they_name():
    """No GPU: the oracle alone on the adversarial batch -- signed zeros survive into the rays, and the negative-zero record exists."""
    sv, keep = six_squares()
    rays, where, _ = adversarial_rays()
    assert len(rays) < 20000 and set(where) == {"axis-parallel, +0 / -0 on the two other axes", "hits on the range bounds", "own axis +0 / -0",
                                                "origin on a plane", "box entered at t == range_t.y", "tmax negative / denormal"}
    dbits = rays["direction"].view(np.uint32)
    for axis in range(3):
        assert (dbits[:, axis] == 0).any() and (dbits[:, axis] == 0x80000000).any()
    ref = po.trace_rays(sv, rays)
    hit = ref["hit"] != 0
    assert (ref["sn"][hit].view(np.uint32) == 0x80000000).any()
    t = rays["tmax"]
    assert (t < 0).any() and ((t > 0) & (t < FLT_MIN)).any()
