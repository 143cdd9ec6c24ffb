"""TRC_FLAG_MESH_LIGHTS on the GPU (tracer_abi.h): the tables and the kernels' sampler bit for bit against the CPU restatement
(tests/meshlight_ref), the refused combinations, scenes without a light triangle = the flag-off frame bit for bit, bit-exact invariances
of the new kernels (fused samples, launch order, block sizes, tiles, image-texture variant, tree residence), sample shards of 4 ranks on
this GPU composed to the frame of the definition, tables that follow the scene
and the triangle materials, the same expectation with and without the mesh's light sample (knob mesh_light_pick), its lower variance, and
a pbrt scene lit by a non-rectangular emissive mesh.  The module renders on a Tracer of its own (the hooks build)."""
import math
import os
import sys

import numpy as np
import pytest

from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "meshlight_ref"))
import meshlight_loader as ml  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MIS = abi.INTEGRATOR_MIS
EMITTER, LAMBERT = 3, 4            # Cornell's material table: the lamp (Diffuse, 11 11 11) and the red wall (Lambert)


@pytest.fixture(scope="module")
def ref():
    return ml.build()


@pytest.fixture(scope="module")
def mgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


# ---------------------------------------------------------------------------------------------------------------- scenes
_SCENES = {}


def flat_shaded(mesh):
    """the same triangles with unshared vertices that carry their triangle's unit geometric normal (degenerate triangles keep theirs)"""
    v, i = mesh.vertices(), mesh.indices()
    out = v[i].copy()
    for t in range(len(i) // 3):
        p = out[3 * t:3 * t + 3, :3].astype(np.float64)
        g = np.cross(p[1] - p[0], p[2] - p[0])
        if np.linalg.norm(g) > 0:
            g /= np.linalg.norm(g)
            out[3 * t:3 * t + 3, 3:6] = g if np.dot(g, out[3 * t:3 * t + 3, 3:6].mean(axis=0)) >= 0 else -g
    return host.Mesh.from_arrays(out, np.arange(len(i), dtype=np.uint32))


def cornell_mesh(name):
    """Cornell box (squareList[5] / [6] present) + a mesh: 'ball' 48 triangles (the whole tree is staged in LDS), 'flatball' the same with
    flat normals, 'bigball' 1104 (read from memory), or a mesh of tests/golden/meshes.npz"""
    if name not in _SCENES:
        mesh = (host.Mesh.ball(4, 6, 0.1) if name == "ball" else flat_shaded(host.Mesh.ball(4, 6, 0.1)) if name == "flatball"
                else host.Mesh.ball(24, 24, 1.0) if name == "bigball" else host.Mesh.golden(name))
        _SCENES[name] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
    return _SCENES[name]


def lamp_materials(n, lamp):
    """every triangle the red Lambert, the triangles `lamp` the emitter"""
    m = np.full(n, LAMBERT, np.uint32)
    m[list(lamp)] = EMITTER
    return m


ROOM_FACES = [  # four corners and the inward normal
    ((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), (0, 1, 0)), ((-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1), (0, -1, 0)),
    ((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1), (1, 0, 0)), ((1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, 0, 0)),
    ((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1), (0, 0, -1)), ((-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1), (0, 0, 1)),
]


def room_pbrt(light_half=0.12, le=40.0, rho=0.6, res=48):
    """A closed Lambert room [-1, 1]^3 of 12 flat-normal triangles and, just below the ceiling, a lamp: a quad of two triangles turned 30
    degrees in its plane (not an axis-aligned rectangle: it stays a mesh).  No square, sphere or cube."""
    P, N, I = [], [], []
    for f in ROOM_FACES:
        b = len(P)
        P += list(f[:4]); N += [f[4]] * 4; I += [b, b + 1, b + 2, b, b + 2, b + 3]
    fl = lambda seq: " ".join(" ".join(repr(float(c)) for c in p) for p in seq)
    c, s, h = math.cos(math.radians(30)), math.sin(math.radians(30)), light_half
    L = [(c * x - s * z, 0.98, s * x + c * z) for x, z in ((-h, -h), (h, -h), (h, h), (-h, h))]
    return f'''LookAt 0 0 -0.95  0 -0.1 0  0 1 0
Camera "perspective" "float fov" [ 75 ]
Film "image" "integer xresolution" [ {res} ] "integer yresolution" [ {res} ]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ {le} {le} {le} ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ {fl(L)} ] "normal N" [ 0 -1 0  0 -1 0  0 -1 0  0 -1 0 ]
AttributeEnd
Material "matte" "rgb Kd" [ {rho} {rho} {rho} ]
Shape "trianglemesh" "integer indices" [ {" ".join(map(str, I))} ] "point P" [ {fl(P)} ] "normal N" [ {fl(N)} ]
WorldEnd
'''


def load_room(tmp_path, **kw):
    p = tmp_path / "room.pbrt"
    p.write_text(room_pbrt(**kw))
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(str(p), triangle_materials=True)
    assert sc.view.n_square == 0 and sc.view.n_index // 3 == 14 and info.n_triangle_material_conflicts == 0
    return sc, cam, info, tri


def setup(t, view, cam, W, H, tri=None, seed=9):
    t.upload_scene(view)
    if tri is not None:
        t.upload_triangle_materials(tri)
    t.set_camera(cam); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    t.seed(seed); t.clear_accum(); t.reset_stats()


def reseed(t, seed=9):
    t.seed(seed); t.clear_accum(); t.reset_stats()


def run(t, spp, calls=1, **kw):
    for c in range(calls):
        t.render(spp=spp, integrator=MIS, frame0=c * spp, **kw)
    return t.download_accum(), t.download_rng()


def same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------- 1. tables and sampler, bit for bit
def test_tables_and_sampler_match_restatement(mgpu, ref):
    rng = np.random.default_rng(17)
    for k, name in enumerate(("teapot", "coatball", "ball")):
        sc = cornell_mesh(name)
        v = sc.view
        n = v.n_index // 3
        # random per-triangle materials over the whole table: ~1/3 of the triangles the emitter, the rest anything (Glass, Metal, checker ...)
        tri_mat = rng.integers(0, v.n_material, size=n).astype(np.uint32)
        tri_mat[rng.random(n) < 0.33] = EMITTER
        mgpu.upload_scene(v)
        mgpu.upload_triangle_materials(tri_mat)
        g = mgpu.mesh_light_tables(n)
        c = ref.tables(ml.view_triangles(v), tri_mat, *ml.view_materials(v))
        assert g["n_lights"] == c["n_lights"] > 0, name
        assert np.array_equal(g["tri"], c["tri"]) and np.array_equal(g["alias"], c["alias"]), name
        assert np.array_equal(g["pdfA"].view(np.uint32), c["pdfA"].view(np.uint32)), name
        assert g["total"] == c["total"], name
        d = ml.edge_draws(rng, 10 ** 6 if k == 0 else 10 ** 5)
        pos = rng.uniform(-300, 800, size=(d.shape[0], 3)).astype(F)
        gt, go = mgpu.mesh_light_test(d, pos)
        ct, co = ref.sample(c, d, pos)
        assert np.array_equal(gt, ct), name
        assert np.array_equal(go.view(np.uint32), co.view(np.uint32)), name
        # without the array every triangle is material 19 (Glass in this table): no light, and the sampler says so
        mgpu.upload_triangle_materials(None)
        g0 = mgpu.mesh_light_tables(n)
        assert g0["n_lights"] == 0 and g0["total"] == 0 and not g0["pdfA"].any()
        with pytest.raises(TracerError) as e:
            mgpu.mesh_light_test(d[:4], pos[:4])
        assert e.value.status == abi.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- 2. refused combinations
def test_refused_combinations(mgpu):
    sc = cornell_mesh("ball")
    n = sc.view.n_index // 3
    setup(mgpu, sc.view, host.prepare_camera(32, 32), 32, 32, lamp_materials(n, (20, 21)))
    mgpu.render(spp=8, integrator=MIS, mesh_lights=True)
    before = mgpu.download_accum(), mgpu.download_rng(), mgpu.stats().as_dict()
    env = np.ones((4, 8, 3), F)
    mgpu.set_environment_map(env)
    try:
        for kw in (dict(integrator=abi.INTEGRATOR_PATH), dict(integrator=abi.INTEGRATOR_VOLUME), dict(integrator=MIS, sobol=True),
                   dict(integrator=MIS, collect_stats=True), dict(integrator=MIS, env_light=True)):
            with pytest.raises(TracerError) as e:
                mgpu.render(spp=8, mesh_lights=True, **kw)
            assert e.value.status == abi.ERR_UNSUPPORTED, kw
    finally:
        mgpu.set_environment_map(None)
    after = mgpu.download_accum(), mgpu.download_rng(), mgpu.stats().as_dict()
    same(before, after)
    for key in ("paths", "rays", "shaded", "launches"):
        assert before[2][key] == after[2][key], key


# ------------------------------------------------------------------------------------------- 3. no light triangle: the flag-off frame
@pytest.mark.parametrize("name", ["ball", "bigball"])
def test_no_light_triangle_equals_flag_off(mgpu, name):
    """p_mesh = 0: every draw and operation of the flag-off kernel (one-wavefront workgroups and on 'bigball' persistent workgroups; a
    96 x 64 frame is too small for a strip launch at any spp: tests/test_gpu_light_oracle.py forces those), with the
    triangles at material 19 and with an array that names no emitter; then knob mesh_light_pick = 0 where the only emitters are squares"""
    sc = cornell_mesh(name)
    n = sc.view.n_index // 3
    cam = host.prepare_camera(96, 64)
    try:
        for tri in (None, lamp_materials(n, ())):
            for spp in (1, 4, 16, 64):
                setup(mgpu, sc.view, cam, 96, 64, tri)
                a = run(mgpu, spp)
                reseed(mgpu)
                b = run(mgpu, spp, mesh_lights=True)
                same(a, b)
                mgpu.debug_set("mesh_light_pick", 0)
                reseed(mgpu)
                same(a, run(mgpu, spp, mesh_lights=True))
                mgpu.debug_set("mesh_light_pick", 1)
    finally:
        mgpu.debug_set("mesh_light_pick", 1)


# ------------------------------------------------------------------------------------------- 4. invariances of the new kernels
@pytest.mark.parametrize("name", ["ball", "bigball"])
def test_invariances(mgpu, name):
    sc = cornell_mesh(name)
    n = sc.view.n_index // 3
    tri = lamp_materials(n, range(n // 3, n // 3 + 6))
    W, H = 96, 64
    cam = host.prepare_camera(W, H)
    setup(mgpu, sc.view, cam, W, H, tri)
    fused = run(mgpu, 16, mesh_lights=True)
    reseed(mgpu)
    same(fused, run(mgpu, 1, calls=16, mesh_lights=True))
    for kw in (dict(fixed_order=True), dict(small_blocks=True), dict(small_blocks=False)):
        reseed(mgpu)
        same(fused, run(mgpu, 16, mesh_lights=True, **kw))
    for ranks in (2, 3):                      # tiles of one context stitch to the whole frame
        reseed(mgpu)
        for r in range(ranks):
            mgpu.render(spp=16, integrator=MIS, tile_rank=r, tile_nranks=ranks, mesh_lights=True)
        same(fused, (mgpu.download_accum(), mgpu.download_rng()))
    # LDS-resident against memory trees: knob no_lds_fit keeps a tree that fits out of LDS
    try:
        mgpu.debug_set("no_lds_fit", 1)
        setup(mgpu, sc.view, cam, W, H, tri)
        same(fused, run(mgpu, 16, mesh_lights=True))
        reseed(mgpu)
        same(fused, run(mgpu, 2, calls=8, mesh_lights=True))
    finally:
        mgpu.debug_set("no_lds_fit", 0)
    # the mesh lights the frame: not the flag-off frame
    setup(mgpu, sc.view, cam, W, H, tri)
    off = run(mgpu, 16)
    assert not np.array_equal(off[0].view(np.uint32), fused[0].view(np.uint32))


def shard_fold(frames, S):
    """tracer_abi.h, sample sharding: the rank-ORDERED binary32 sum of the ranks' accumulators, one IEEE division by S"""
    acc = frames[0]
    for a in frames[1:]:
        acc = np.add(acc, a, dtype=np.float32)
    return np.divide(acc, np.float32(S), dtype=np.float32)


def run_mesh_ranks(world, outdir, name):
    """`world` processes on this GPU, each tests/_meshlight_rank_worker.py (collectives over gloo, as tests/test_gpu_shared_gpu_ranks.py)"""
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(outdir, exist_ok=True)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TRC_ROOT=root, TRC_OUT=str(outdir), TRC_MESH=name, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "_meshlight_rank_worker.py")], env=env))
    import time
    deadline = time.monotonic() + 600            # one deadline for all ranks; the first rank that fails ends the wait, and `finally` the others
    try:
        waiting = list(procs)
        while waiting:
            for p in list(waiting):
                rc = p.poll()
                if rc is not None:
                    assert rc == 0, f"a rank of {world} failed with {rc}"
                    waiting.remove(p)
            assert time.monotonic() < deadline, f"{len(waiting)} of {world} ranks still running at the deadline"
            time.sleep(0.05)
    finally:
        for p in procs:                      # our own children, by PID
            if p.poll() is None:
                p.kill()
    return [np.load(os.path.join(outdir, f"rank{r}.npz")) for r in range(world)]


SHARD_W, SHARD_H, SHARD_SPP = 96, 64, 16


def shard_lamp(n):
    return lamp_materials(n, range(n // 3, n // 3 + 6))


@pytest.mark.parametrize("name", ["ball", "bigball"])
def test_sample_shards_compose_to_the_defined_frame(mgpu, tmp_path, name):
    """Sample sharding (tracer_abi.h) under TRC_FLAG_MESH_LIGHTS, on a scene with six light triangles beside the squares (p_mesh = 1/2: the
    mesh's four extra draws are on the path).  4 ranks share this GPU: trc_group_compose_samples over 4 sample groups, then over 2 sample
    groups x 2 tile ranks (pipelined), then the every-rank compose; group g renders from trc_seed(trc_shard_seed(seed, g)), flag on.
    The expected frame is the definition, built as the existing shard tests build it: this GPU renders the groups' whole frames one after
    the other from the same seeds, folded in rank order in binary32 and divided by S.  (There is no oracle for a mesh light: the frames of
    one context are held to the invariances above and to the CPU restatement of tables and sampler.)"""
    world = 4
    sc = cornell_mesh(name)
    n = sc.view.n_index // 3
    res = run_mesh_ranks(world, tmp_path / "ranks", name)
    setup(mgpu, sc.view, host.prepare_camera(SHARD_W, SHARD_H), SHARD_W, SHARD_H, shard_lamp(n))
    assert mgpu.mesh_light_tables(n)["n_lights"] == 6

    def group_frames(seed, S):
        out = []
        for g in range(S):
            reseed(mgpu, abi.shard_seed(seed, g))
            out.append(run(mgpu, SHARD_SPP // S, mesh_lights=True)[0])
        return out

    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    four = group_frames(100, 4)
    want = shard_fold(four, 4)
    assert (want[..., 3] == 1).all() and not np.array_equal(bits(four[0]), bits(four[1]))
    assert np.array_equal(bits(res[0]["samples"]), bits(want))
    for r in range(world):
        assert np.array_equal(bits(res[r]["own"]), bits(four[r])), r          # every rank rendered its group's frame
        assert np.array_equal(bits(res[r]["mean"]), bits(want)), r            # trc_group_allreduce_mean_accum: on every rank
        assert int(res[r]["n_lights"]) == 6, r
    # S = 2 sample groups x T = 2 tile ranks: rank r is tile rank r % 2 of group r // 2; the zeros of the other tile rank are exact
    # identities of the sum, so the fold of the 4 accumulators is the fold of the 2 groups' whole frames
    two = group_frames(200, 2)
    assert np.array_equal(bits(res[0]["hybrid"]), bits(shard_fold(two, 2)))
    # flag off, the same shards give another frame: the flag was on in the ranks
    reseed(mgpu, abi.shard_seed(100, 1))
    assert not np.array_equal(bits(run(mgpu, SHARD_SPP // 4)[0]), bits(res[1]["own"]))


@pytest.mark.parametrize("name", ["ball", "bigball"])
def test_image_texture_variant_agrees(mgpu, name):
    """k_render*_mesh<.., TEX>: uniform images on every non-emitter material against the same colours as Constant textures"""
    import ctypes as C
    base = cornell_mesh(name).view
    n = base.n_index // 3
    tri = lamp_materials(n, range(n // 3, n // 3 + 6))
    tex_m, const_m = (abi.Material * base.n_material)(), (abi.Material * base.n_material)()
    imgs = []
    for i in range(base.n_material):
        tex_m[i] = base.materials[i]; const_m[i] = base.materials[i]
        if base.materials[i].type == abi.MAT_DIFFUSE:
            continue
        c = (0.5, 0.25, 0.125)
        imgs.append(np.broadcast_to(np.array(c, F), (3, 5, 3)).copy())
        tex_m[i].textureInfo.type = abi.TEX_IMAGE
        tex_m[i].textureInfo.textureIndex = len(imgs) - 1
        const_m[i].textureInfo.type = abi.TEX_CONSTANT
        const_m[i].textureInfo.albedo.x, const_m[i].textureInfo.albedo.y, const_m[i].textureInfo.albedo.z = c
    views = []
    for mats in (tex_m, const_m):
        v = abi.Scene.from_buffer_copy(base)
        v.materials = C.cast(mats, C.POINTER(abi.Material))
        views.append(v)
    cam = host.prepare_camera(64, 64)
    try:
        for spp in (2, 16):
            setup(mgpu, views[0], cam, 64, 64, tri); mgpu.upload_textures(imgs)
            a = run(mgpu, spp, mesh_lights=True)
            setup(mgpu, views[1], cam, 64, 64, tri); mgpu.upload_textures([])
            same(a, run(mgpu, spp, mesh_lights=True))
    finally:
        mgpu.upload_textures([])


# ------------------------------------------------------------------------------------------- 5. tables follow the scene
def test_tables_follow_triangle_materials(mgpu):
    sc = cornell_mesh("ball")
    n = sc.view.n_index // 3
    cam = host.prepare_camera(64, 48)
    first, second = lamp_materials(n, (4, 5, 6)), lamp_materials(n, (30, 31))

    def fresh(tri, **kw):
        with Tracer(0) as t:
            setup(t, sc.view, cam, 64, 48, tri)
            return run(t, 16, **kw)

    setup(mgpu, sc.view, cam, 64, 48, first)
    a = run(mgpu, 16, mesh_lights=True)
    mgpu.upload_triangle_materials(second)                   # the emitter moves to another set of triangles
    assert list(mgpu.mesh_light_tables(n)["tri"]) == [30, 31]
    reseed(mgpu)
    b = run(mgpu, 16, mesh_lights=True)
    same(b, fresh(second, mesh_lights=True))
    assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    mgpu.upload_triangle_materials(None)                     # material 19 everywhere: no light triangle
    assert mgpu.mesh_light_tables(n)["n_lights"] == 0
    reseed(mgpu)
    c = run(mgpu, 16, mesh_lights=True)
    same(c, fresh(None, mesh_lights=True))
    same(c, fresh(None))
    mgpu.upload_scene(cornell_mesh("bigball").view)          # another scene: its own tables
    assert mgpu.mesh_light_tables(cornell_mesh("bigball").view.n_index // 3)["n_lights"] == 0


# ------------------------------------------------------------------------------------------- 6. / 7. expectation and variance
def seeds_of_frames(t, K, spp, blocks, seed0, **kw):
    """K independent frames (seeds seed0 .. seed0 + K - 1) -> (K, blocks, blocks, 3) means over image blocks of pixels"""
    out = []
    for k in range(K):
        reseed(t, seed0 + k)
        a = run(t, spp, **kw)[0][..., :3].astype(np.float64)
        H, W = a.shape[:2]
        out.append(a.reshape(blocks, H // blocks, blocks, W // blocks, 3).mean(axis=(1, 3)))
    return np.array(out)


def expectation_check(t, K, spp, blocks):
    """flag-on against flag-on with mesh_light_pick = 0 (the BSDF-only estimator of the same integrand): per block and channel, the means
    of K seeds within 6 combined standard errors, the errors estimated from the K frames themselves.  The two arms take disjoint seed sets
    (1000 .. and 5000 ..): with shared seeds they would share every camera ray and first vertex, the arms would be positively correlated,
    and the sum of the two variances would overstate the spread of the difference -- a bound looser than its nominal 6"""
    try:
        on = seeds_of_frames(t, K, spp, blocks, 1000, mesh_lights=True)
        t.debug_set("mesh_light_pick", 0)
        bsdf = seeds_of_frames(t, K, spp, blocks, 5000, mesh_lights=True)
    finally:
        t.debug_set("mesh_light_pick", 1)
    se = np.sqrt(on.var(axis=0, ddof=1) / K + bsdf.var(axis=0, ddof=1) / K)
    mean = 0.5 * (on.mean(axis=0) + bsdf.mean(axis=0))
    z = (on.mean(axis=0) - bsdf.mean(axis=0)) / se
    rel = se / mean
    print(f"expectation: K {K}, spp {spp}, {blocks} x {blocks} blocks: combined se / mean median {np.median(rel):.4f} max {rel.max():.4f}; "
          f"|z| max {np.abs(z).max():.2f}, z mean {z.mean():+.3f}; frame mean on {on.mean():.5f} bsdf-only {bsdf.mean():.5f}")
    assert (mean > 0).all() and (se > 0).all()
    assert np.abs(z).max() < 6, z
    return rel


def test_expectation_closed_room(mgpu, tmp_path):
    """The closed room lit by the mesh lamp alone (no squares: p_mesh = 1).  K = 16 seeds x 1024 spp at 48 x 48, 4 x 4 blocks of 144 pixels.
    Measured on an MI355X: combined standard error / mean per block and channel: median 0.0108, max 0.0169; |z| max 2.54."""
    sc, cam, info, tri = load_room(tmp_path)
    setup(mgpu, sc.view, cam, info.xres, info.yres, tri)
    assert mgpu.mesh_light_tables(14)["n_lights"] == 2
    expectation_check(mgpu, 16, 1024, 4)


def test_expectation_cornell(mgpu):
    """The Cornell box (squareList[5] / [6] sampled with probability 1/2 each side of p_mesh = 1/2) + the flat-shaded ball with a quad of
    two emissive triangles.  K = 16 seeds x 1024 spp at 64 x 64, 4 x 4 blocks of 256 pixels.  Measured on an MI355X: combined standard error /
    mean per block and channel: median 0.0087, max 0.0290; |z| max 2.42, whole-frame means 0.07827 / 0.07828.  Flat normals on purpose: under interpolated normals the reference shades in the frame of
    the UNNORMALISED normal (Triangle.hh, B-5), where its BSDF sample and its F / pdf are not one density, so a light sample and a BSDF
    sample do not estimate the same integrand there -- with or without this flag."""
    sc = cornell_mesh("flatball")
    n = sc.view.n_index // 3
    setup(mgpu, sc.view, host.prepare_camera(64, 64), 64, 64, lamp_materials(n, (20, 21)))
    assert mgpu.mesh_light_tables(n)["n_lights"] == 2
    expectation_check(mgpu, 16, 1024, 4)


def test_variance_lower_with_mesh_sampling(mgpu, tmp_path):
    """Equal spp (16), the closed room with a lamp of 0.24 x 0.24 under a 2 x 2 ceiling: mean squared error against a 16384-spp
    mesh_light_pick = 0 render, with the mesh's light sample over without it.  Measured on an MI355X: 0.0152 over 0.2132, ratio 0.0715 (asserted: < 1)."""
    sc, cam, info, tri = load_room(tmp_path)
    W, H = info.xres, info.yres
    setup(mgpu, sc.view, cam, W, H, tri)
    try:
        mgpu.debug_set("mesh_light_pick", 0)
        reseed(mgpu, 77)
        long = run(mgpu, 1024, calls=16, mesh_lights=True)[0][..., :3].astype(np.float64)
        mse = {}
        for pick in (0, 1):
            mgpu.debug_set("mesh_light_pick", pick)
            err = []
            for k in range(4):
                reseed(mgpu, 300 + k)
                f = run(mgpu, 16, mesh_lights=True)[0][..., :3].astype(np.float64)
                err.append(((f - long) ** 2).mean())
            mse[pick] = float(np.mean(err))
    finally:
        mgpu.debug_set("mesh_light_pick", 1)
    print(f"equal-spp (16) MSE against a 16384-spp BSDF-only render: BSDF only {mse[0]:.6g}, with the mesh's light sample {mse[1]:.6g}, "
          f"ratio {mse[1] / mse[0]:.4f}")
    assert mse[1] / mse[0] < 1, mse


# ------------------------------------------------------------------------------------------- 8. a pbrt scene lit by a mesh
FAN_PBRT = '''LookAt 0 1.5 -3  0 0.3 0  0 1 0
Camera "perspective" "float fov" [ 50 ]
Film "image" "integer xresolution" [ 64 ] "integer yresolution" [ 48 ]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 20 16 12 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2  0 2 3  0 3 4 ]
        "point P" [ 0 2 0  0.5 2.2 -0.3  0.6 2.1 0.4  -0.2 2.3 0.6  -0.6 2 0.1 ]
AttributeEnd
Material "matte" "rgb Kd" [ 0.7 0.6 0.5 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -5 0 -5  5 0 -5  5 0 5  -5 0 5 ]
      "normal N" [ 0 1 0  0 1 0  0 1 0  0 1 0 ]
Material "matte" "rgb Kd" [ 0.2 0.5 0.7 ]
Shape "trianglemesh" "integer indices" [ 0 1 2  0 2 3  0 3 1  1 3 2 ] "point P" [ 0 0.9 0  0.5 0 -0.4  -0.5 0 -0.4  0 0 0.5 ]
WorldEnd
'''


def test_pbrt_scene_lit_by_a_mesh(mgpu, tmp_path):
    p = tmp_path / "fan.pbrt"
    p.write_text(FAN_PBRT)
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(str(p), triangle_materials=True)
    assert info.mis_ready == 0                                    # no rectangular area light: flag-off traceMIS refuses the scene
    setup(mgpu, sc.view, cam, info.xres, info.yres, tri)
    with pytest.raises(TracerError) as e:
        mgpu.render(spp=8, integrator=MIS)
    assert e.value.status == abi.ERR_INVALID_ARG
    t = mgpu.mesh_light_tables(sc.view.n_index // 3)
    assert t["n_lights"] == 3 and list(t["tri"]) == [0, 1, 2]
    a = run(mgpu, 64, mesh_lights=True)[0][..., :3]
    assert np.isfinite(a).all() and a.min() >= 0
    assert (a.max(axis=2) > 0).mean() > 0.5 and a.mean() > 0.01  # lit: most pixels see the floor or the lamp
    mgpu.upload_triangle_materials(None)
