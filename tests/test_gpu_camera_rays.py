"""TRC_FLAG_CAMERA_RAYS (include/tracer_abi.h): a sample's camera ray is read from the context's camera-ray sets.  Nothing else about a
sample changes, so the feature is held to the existing kernels, which are held to the oracle: with the camera's own rays a flagged render
IS the unflagged one, bit for bit (identity); with a permutation of them it is a permuted frame (permutation: wrong indexing, a wrong
set or a ray made another way show here); with two sets it is the unflagged sample chain with every pixel's state moved to where its ray
lives (set selection).  Then: the device generator against its host definition, the flag under a tile mask / tile ranks /
trc_render_adaptive, and state and refusals.

Scenes of the kernel census (light_oracle_cases.cornell): Cornell + the 48-triangle ball (the tree in LDS) or the 1104-triangle one (read
from memory), 61 x 45, 8 samples, the camera of prepare_camera (lens radius 0, no zero component in lookFrom), a constant environment that
is not black.  Everything is compared as uint32.  After a launch that left an error behind nothing more of this module runs on the GPU."""
import ctypes as C

import numpy as np
import pytest

import light_oracle_cases as lc
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu

W, H, SEED, SPP = lc.W, lc.H, lc.SEED, 8
N = W * H
INTEGRATORS = {"path": lc.PATH, "mis": lc.MIS}
FAULTED = []
_PLAIN = {}                 # (residence, integrator) -> the unflagged frame of the scene without images and with material 19 on the mesh


@pytest.fixture(scope="module")
def rgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def u32(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)


def _upload(t, s, w=W, h=H, cam=None):
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    t.upload_scene(s.view); t.upload_triangle_materials(s.tri); t.upload_textures(s.images)
    t.set_camera(cam if cam is not None else s.cam); t.set_environment(lc.ENV_RGB); t.set_environment_map(None); t.resize(w, h)


def _frame(t, what, integrator, flagged, spp=SPP, calls=1, frame0=0, rng=None, accum=None, reset=True, **kw):
    """seed (or upload) the RNG texture, clear (or upload) the accumulator, `calls` launches of spp / calls samples -> (accum, rng, stats)"""
    try:
        t.seed(SEED) if rng is None else t.upload_rng(np.ascontiguousarray(rng))
        t.clear_accum() if accum is None else t.upload_accum(np.ascontiguousarray(accum))
        if reset:
            t.reset_stats()
        for c in range(calls):
            t.render(spp=spp // calls, integrator=integrator, frame0=frame0 + c * (spp // calls), camera_rays=flagged, **kw)
        st = t.stats()
        return t.download_accum(), t.download_rng(), (st.rays, st.paths, st.shaded)
    except TracerError:
        FAULTED.append(what)
        raise


def _same(got, want, what):
    bad = np.argwhere((got[0].view(np.uint32) != want[0].view(np.uint32)).any(axis=-1))
    print(f"{what}: accum mismatches {len(bad)}, rng mismatches {int((got[1] != want[1]).any(axis=-1).sum())}, stats {got[2]} / {want[2]}")
    assert np.isfinite(got[0]).all()
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first (y, x) {bad[0]}"
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _plain(t, residence, name):
    """the unflagged 8-sample frame of the plain scene of a residence (cached): what tests 2, 5 and 6 compare with"""
    if (residence, name) not in _PLAIN:
        _upload(t, lc.cornell(residence, False, False))
        _PLAIN[(residence, name)] = _frame(t, f"plain-{residence}-{name}", INTEGRATORS[name], False)
    return _PLAIN[(residence, name)]


def _permutation(kind):
    if kind == "mirror":
        ys, xs = np.mgrid[0:H, 0:W]
        return (ys * W + (W - 1 - xs)).ravel()
    return np.random.default_rng(31).permutation(N)


def _host_rays(s, pi=None):
    rays = host.generate_camera_rays(s.cam, W, H)[0]
    return rays if pi is None else np.ascontiguousarray(rays.ravel()[pi].reshape(H, W))


# ---------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("tex", (False, True), ids=("notex", "tex"))
@pytest.mark.parametrize("trimat", (False, True), ids=("plain19", "trimat"))
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_the_cameras_own_rays_give_the_unflagged_render(rgpu, residence, trimat, tex):
    """(On a library that ignores the flag bit this alone would show nothing: generate_camera_rays and last_camera_rays are what fail there.)"""
    t, s = rgpu, lc.cornell(residence, tex, trimat)
    _upload(t, s)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
    for name, integ in INTEGRATORS.items():
        for calls in (1, SPP):              # 8 samples in one call; 8 calls of 1 sample, coalesced
            what = f"{residence}-{'trimat' if trimat else 'plain19'}-{'tex' if tex else 'notex'}-{name}-{calls}x{SPP // calls}"
            want = _frame(t, what, integ, False, calls=calls)
            assert not t.last_camera_rays()
            got = _frame(t, what, integ, True, calls=calls)
            k = t.last_kernel()
            assert t.last_camera_rays() and k["shape"] == "one" and k["variant"] == ("tex" if tex else "plain") and k["strip"] == 1, k
            assert k["lds_resident"] == (residence == "lds") and k["triangle_materials"] == trimat, k
            assert want[2][1] == N * SPP
            _same(got, want, what)


# ---------------------------------------------------------------------- 2. permutation
@pytest.mark.parametrize("residence,name,kind", [(r, n, "random") for r in ("lds", "mem") for n in INTEGRATORS] + [("lds", "path", "mirror")])
def test_permuted_rays_give_the_permuted_frame(rgpu, residence, name, kind):
    t, s = rgpu, lc.cornell(residence, False, False)
    plain = _plain(t, residence, name)
    pi = _permutation(kind)
    assert np.array_equal(np.sort(pi), np.arange(N)) and (pi != np.arange(N)).sum() > N // 2
    _upload(t, s)
    t.upload_camera_rays(_host_rays(s, pi))                                     # pixel p holds the ray of pi(p) ...
    rng = host.fill_rng(SEED, W, H).reshape(N, 4)[pi].reshape(H, W, 4)          # ... and its RNG texel
    acc, rng_out, st = _frame(t, f"perm-{residence}-{name}-{kind}", INTEGRATORS[name], True, rng=rng)
    assert t.last_camera_rays()
    want = (plain[0].reshape(N, 4)[pi].reshape(H, W, 4), plain[1].reshape(N, 4)[pi].reshape(H, W, 4), plain[2])
    assert (want[0].view(np.uint32) != plain[0].view(np.uint32)).any(axis=-1).sum() > N // 2      # the permuted frame is another frame
    _same((acc, rng_out, st), want, f"perm-{residence}-{name}-{kind}")


# ---------------------------------------------------------------------- 3. set selection
@pytest.mark.parametrize("frame0", (0, 1))
def test_sample_s_takes_set_frame0_plus_s_modulo_n_sets(rgpu, frame0):
    """Two sets: 0 the camera's own rays, 1 their permutation.  One flagged call of 4 samples against four unflagged calls of 1 sample,
    between which every pixel's accumulator and RNG texel are moved to the pixel whose camera ray it takes next, and back."""
    t, s = rgpu, lc.cornell("lds", False, False)
    pi = _permutation("random")
    inv = np.argsort(pi)
    _upload(t, s)
    t.upload_camera_rays(np.stack([_host_rays(s), _host_rays(s, pi)]))
    got = _frame(t, f"sets-{frame0}", lc.MIS, True, spp=4, frame0=frame0)
    assert t.last_camera_rays()
    acc, rng = np.zeros((H, W, 4), np.float32), host.fill_rng(SEED, W, H)
    t.reset_stats()
    for smp in range(4):
        k = (frame0 + smp) % 2
        if k:       # the state of pixel p goes to pixel pi(p), whose camera ray p takes
            acc, rng = acc.reshape(N, 4)[inv].reshape(H, W, 4), rng.reshape(N, 4)[inv].reshape(H, W, 4)
        acc, rng, st = _frame(t, f"sets-{frame0}-ref", lc.MIS, False, spp=1, frame0=frame0 + smp, rng=rng, accum=acc, reset=False)
        if k:
            acc, rng = acc.reshape(N, 4)[pi].reshape(H, W, 4), rng.reshape(N, 4)[pi].reshape(H, W, 4)
    _same(got, (acc, rng, st), f"sets-{frame0}")


# ---------------------------------------------------------------------- 4. the device generator equals its definition
@pytest.mark.parametrize("size", ((W, H), (1, 1), (7, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_generator_equals_the_host_definition(rgpu, size):
    t, s = rgpu, lc.cornell("lds", False, False)
    w, h = size
    cam = host.prepare_camera(w, h)
    _upload(t, s, w, h, cam)
    offsets = np.array([[0.0, 0.0], [0.5, 0.5], host.halton_offsets(2)[1]], np.float32)
    try:
        for model in (abi.RAYS_PINHOLE, abi.RAYS_ORTHOGRAPHIC, abi.RAYS_EQUIRECT):
            want = host.generate_camera_rays(cam, w, h, model, 3, offsets)
            t.generate_camera_rays(model, 3, offsets)
            for k in range(3):
                got = t.download_camera_rays(k)
                bad = int((u32(got) != u32(want[k])).sum())
                print(f"{w}x{h} model {model} set {k}: {bad} of {8 * w * h} words differ")
                assert bad == 0
            assert np.isfinite(want["direction"]).all() and (want["tmax"] == np.finfo(np.float32).max).all() and not want["_pad"].any()
        t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)          # offsets == NULL is all zero
        assert np.array_equal(u32(t.download_camera_rays(0)), u32(host.generate_camera_rays(cam, w, h, abi.RAYS_PINHOLE, 1, np.zeros((1, 2), np.float32))[0]))
    except TracerError:
        FAULTED.append(f"generator-{w}x{h}")
        raise


# ---------------------------------------------------------------------- 5. composition
def test_tile_mask_tile_ranks_and_adaptive_passes(rgpu):
    t, s = rgpu, lc.cornell("mem", False, False)
    _upload(t, s)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 4, host.halton_offsets(4))
    whole = _frame(t, "compose-whole", lc.MIS, True)
    assert t.last_camera_rays()
    assert (whole[0].view(np.uint32) != _plain(t, "mem", "mis")[0].view(np.uint32)).any()          # offsets: another picture
    _upload(t, s)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 4, host.halton_offsets(4))
    # a mask that keeps about half the tiles: the others' accumulator and RNG texels stay as they were
    rows, cols = t.tile_grid()
    mask = (np.add.outer(np.arange(rows), np.arange(cols)) % 2 == 0)
    ys, xs = np.mgrid[0:H, 0:W] // abi.TRC_TILE
    kept = mask[ys, xs]
    try:
        t.set_tile_mask(mask)
        acc, rng, st = _frame(t, "compose-mask", lc.MIS, True)
        t.set_tile_mask(None)
    except TracerError:
        FAULTED.append("compose-mask")
        raise
    assert 0 < kept.sum() < N and st[1] == kept.sum() * SPP
    assert np.array_equal(acc[kept].view(np.uint32), whole[0][kept].view(np.uint32)) and np.array_equal(rng[kept], whole[1][kept])
    assert not acc[~kept].view(np.uint32).any() and np.array_equal(rng[~kept], host.fill_rng(SEED, W, H)[~kept])
    # two tile ranks assemble the whole frame
    try:
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        for rank in (0, 1):
            t.render(spp=SPP, integrator=lc.MIS, tile_rank=rank, tile_nranks=2, camera_rays=True)
            assert t.last_camera_rays()
        st = t.stats()
        _same((t.download_accum(), t.download_rng(), (st.rays, st.paths, st.shaded)), whole, "compose-ranks")
        # trc_render_adaptive with the flag in p->flags
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        rep = t.render_adaptive(threshold=0.05, max_spp=32, spp=8, integrator=lc.MIS, flags=abi.FLAG_CAMERA_RAYS)
        assert t.last_camera_rays()
        paths = t.stats().paths
        print(f"adaptive: {rep.as_dict()}, paths {paths}")
        assert rep.passes >= 2 and rep.samples == paths and N * 16 <= paths <= N * 32
        assert np.isfinite(t.download_accum()).all()
    except TracerError:
        FAULTED.append("compose")
        raise


# ---------------------------------------------------------------------- 6. state and refusals
def _refused(fn, status):
    with pytest.raises(TracerError) as e:
        fn()
    assert e.value.status == status, e.value


def test_state_and_refusals(rgpu):
    t, s = rgpu, lc.cornell("lds", False, False)
    plain = _plain(t, "lds", "mis")
    _upload(t, s)
    t.seed(SEED); t.clear_accum()
    before = t.download_accum(), t.download_rng()

    def unchanged():
        assert np.array_equal(u32(t.download_accum()), u32(before[0])) and np.array_equal(t.download_rng(), before[1])
    flagged = lambda **kw: t.render(**{**dict(spp=SPP, integrator=lc.MIS, camera_rays=True), **kw})
    _refused(flagged, abi.ERR_UNSUPPORTED)                                                   # the flag without rays
    _refused(lambda: t.download_camera_rays(0), abi.ERR_NO_FRAME)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 2, None)
    _refused(lambda: flagged(integrator=lc.VOLUME), abi.ERR_UNSUPPORTED)
    for kw in (dict(sobol=True), dict(collect_stats=True), dict(env_light=True), dict(mesh_lights=True), dict(view_height=15)):
        _refused(lambda: flagged(**kw), abi.ERR_UNSUPPORTED)
    _refused(lambda: t.render_adaptive(threshold=0.05, max_spp=32, spp=8, integrator=lc.VOLUME, flags=abi.FLAG_CAMERA_RAYS), abi.ERR_UNSUPPORTED)
    unchanged()
    # bad arguments
    L, h = t._L, t._h
    g = abi.RayGen(model=abi.RAYS_PINHOLE, n_sets=1)
    assert L.trc_generate_camera_rays(h, None) == abi.ERR_INVALID_ARG and L.trc_upload_camera_rays(h, None, 1) == abi.ERR_INVALID_ARG
    assert L.trc_download_camera_rays(h, 0, None) == abi.ERR_INVALID_ARG
    for n_sets in (0, abi.TRC_MAX_RAY_SETS + 1):
        g.n_sets = n_sets
        assert L.trc_generate_camera_rays(h, C.byref(g)) == abi.ERR_INVALID_ARG
        assert L.trc_upload_camera_rays(h, host.generate_camera_rays(s.cam, W, H).ctypes.data, n_sets) == abi.ERR_INVALID_ARG
    _refused(lambda: t.generate_camera_rays(3, 1, None), abi.ERR_INVALID_ARG)
    for bad in (1.0, -0.25, np.nan, np.inf):
        _refused(lambda: t.generate_camera_rays(abi.RAYS_PINHOLE, 2, np.array([[0.0, 0.5], [bad, 0.0]], np.float32)), abi.ERR_INVALID_ARG)
    _refused(lambda: t.download_camera_rays(2), abi.ERR_INVALID_ARG)
    assert len(t.download_camera_rays(1)) == H                                               # the refused calls left the two sets in force
    # a scene upload and a camera keep the rays; trc_resize and trc_clear_camera_rays drop them
    t.upload_scene(s.view); t.set_camera(s.cam)
    try:
        flagged()
        assert t.last_camera_rays()
        _same(_frame(t, "after-refusals-flagged", lc.MIS, True), plain, "the rays survive trc_upload_scene and trc_set_camera")
        t.clear_camera_rays()
        _refused(flagged, abi.ERR_UNSUPPORTED)
        t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
        t.resize(W, H)
        _refused(flagged, abi.ERR_UNSUPPORTED)
        _refused(lambda: t.download_camera_rays(0), abi.ERR_NO_FRAME)
        _same(_frame(t, "after-refusals", lc.MIS, False), plain, "an unflagged render after the refusals")
        assert not t.last_camera_rays()
    except TracerError:
        FAULTED.append("state")
        raise
    # before trc_resize, and before trc_set_camera
    with Tracer(0, hooks=True) as fresh:
        _refused(lambda: fresh.generate_camera_rays(abi.RAYS_PINHOLE, 1, None), abi.ERR_NO_FRAME)
        _refused(fresh.clear_camera_rays, abi.ERR_NO_FRAME)
        assert fresh._L.trc_upload_camera_rays(fresh._h, host.generate_camera_rays(s.cam, W, H).ctypes.data, 1) == abi.ERR_NO_FRAME
        fresh.resize(W, H)
        _refused(lambda: fresh.generate_camera_rays(abi.RAYS_PINHOLE, 1, None), abi.ERR_INVALID_ARG)
