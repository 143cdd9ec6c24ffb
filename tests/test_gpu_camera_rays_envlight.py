"""TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT (include/tracer_abi.h): a sample takes its camera ray from the context's ray sets, and
everything after that is the TRC_FLAG_ENV_LIGHT sample.  The unflagged TRC_FLAG_ENV_LIGHT launch is held to the oracle by
tests/test_gpu_light_oracle.py, so it is the reference here, as the unflagged kernels are in tests/test_gpu_camera_rays.py: with the
camera's own rays the pair IS that launch bit for bit (all eight k_render_rays_env kernels: two residences, image textures, the
per-triangle-material twins); with permuted rays it is the permuted frame; with two sets it is the unflagged sample chain with every
pixel's state moved to where its ray lives; an equirectangular set renders, and lights every pixel whose ray leaves the scene; the
refusals are the union of the two flags'; a tile mask and trc_render_adaptive compose.

Scenes of tests/light_oracle_cases.py: Cornell + the 48-triangle ball (the tree in LDS) or the 1104-triangle one (read from memory),
61 x 45, 8 samples, its "sun" map.  Everything is compared as uint32.  After a launch that left an error behind nothing more of this
module runs on the GPU."""
import numpy as np
import pytest

import light_oracle_cases as lc
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu

W, H, SEED, SPP = lc.W, lc.H, lc.SEED, 8
N = W * H
FAULTED = []
_ENV = {}                   # residence -> the unflagged env-lit frame of the scene without images and with material 19 on the mesh


@pytest.fixture(scope="module")
def rgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def u32(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)


def _upload(t, s, cam=None, env="sun"):
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    t.upload_scene(s.view); t.upload_triangle_materials(s.tri); t.upload_textures(s.images)
    t.set_camera(cam if cam is not None else s.cam); t.set_environment((0.0, 0.0, 0.0))
    t.set_environment_map(lc.env_map(env) if env else None); t.resize(W, H)


def _frame(t, what, flagged, spp=SPP, calls=1, frame0=0, rng=None, accum=None, reset=True, **kw):
    """seed (or upload) the RNG texture, clear (or upload) the accumulator, `calls` traceMIS launches of spp / calls samples under
    TRC_FLAG_ENV_LIGHT -> (accum, rng, stats)"""
    try:
        t.seed(SEED) if rng is None else t.upload_rng(np.ascontiguousarray(rng))
        t.clear_accum() if accum is None else t.upload_accum(np.ascontiguousarray(accum))
        if reset:
            t.reset_stats()
        for c in range(calls):
            t.render(spp=spp // calls, integrator=lc.MIS, frame0=frame0 + c * (spp // calls), env_light=True, camera_rays=flagged, **kw)
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


def _env_plain(t, residence):
    """the unflagged env-lit 8-sample frame of the plain scene of a residence (cached): what tests 2 and 6 compare with"""
    if residence not in _ENV:
        _upload(t, lc.cornell(residence, False, False))
        _ENV[residence] = _frame(t, f"env-plain-{residence}", False)
        assert t.last_kernel()["variant"] == "env" and not t.last_camera_rays()
    return _ENV[residence]


def _host_rays(s, pi=None):
    rays = host.generate_camera_rays(s.cam, W, H)[0]
    return rays if pi is None else np.ascontiguousarray(rays.ravel()[pi].reshape(H, W))


def _permute(a, pi):
    return a.reshape(N, 4)[pi].reshape(H, W, 4)


PI = np.random.default_rng(31).permutation(N)


# ---------------------------------------------------------------------- 1. identity: all eight kernels
@pytest.mark.parametrize("tex", (False, True), ids=("notex", "tex"))
@pytest.mark.parametrize("trimat", (False, True), ids=("plain19", "trimat"))
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_the_cameras_own_rays_give_the_unflagged_env_lit_render(rgpu, residence, trimat, tex):
    t, s = rgpu, lc.cornell(residence, tex, trimat)
    _upload(t, s)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
    for calls in (1, SPP):                  # 8 samples in one call; 8 calls of 1 sample, coalesced
        what = f"{residence}-{'trimat' if trimat else 'plain19'}-{'tex' if tex else 'notex'}-{calls}x{SPP // calls}"
        want = _frame(t, what, False, calls=calls)
        assert not t.last_camera_rays() and t.last_kernel()["variant"] == ("env_tex" if tex else "env")
        got = _frame(t, what, True, calls=calls)
        k = t.last_kernel()
        assert t.last_camera_rays() and k["shape"] == "one" and k["variant"] == ("env_tex" if tex else "env") and k["strip"] == 1, k
        assert k["lds_resident"] == (residence == "lds") and k["triangle_materials"] == trimat, k
        assert want[2][1] == N * SPP
        _same(got, want, what)


# ---------------------------------------------------------------------- 2. permutation
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_permuted_rays_give_the_permuted_frame(rgpu, residence):
    t, s = rgpu, lc.cornell(residence, False, False)
    plain = _env_plain(t, residence)
    assert np.array_equal(np.sort(PI), np.arange(N)) and (PI != np.arange(N)).sum() > N // 2
    _upload(t, s)
    t.upload_camera_rays(_host_rays(s, PI))                                     # pixel p holds the ray of pi(p) ...
    rng = _permute(host.fill_rng(SEED, W, H), PI)                               # ... and its RNG texel
    got = _frame(t, f"perm-{residence}", True, rng=rng)
    assert t.last_camera_rays() and t.last_kernel()["variant"] == "env"
    want = (_permute(plain[0], PI), _permute(plain[1], PI), plain[2])
    assert (want[0].view(np.uint32) != plain[0].view(np.uint32)).any(axis=-1).sum() > N // 2      # the permuted frame is another frame
    _same(got, want, f"perm-{residence}")


# ---------------------------------------------------------------------- 3. two sets and frame0
@pytest.mark.parametrize("frame0", (0, 1))
def test_sample_s_takes_set_frame0_plus_s_modulo_2(rgpu, frame0):
    """Two sets: 0 the camera's own rays, 1 their permutation.  One flagged call of 8 samples, and 8 flagged calls of 1, against eight
    unflagged env-lit calls of 1 sample, between which every pixel's accumulator and RNG texel are moved to the pixel whose camera ray it
    takes next, and back."""
    t, s = rgpu, lc.cornell("lds", False, False)
    inv = np.argsort(PI)
    _upload(t, s)
    t.upload_camera_rays(np.stack([_host_rays(s), _host_rays(s, PI)]))
    one = _frame(t, f"sets-{frame0}-1x8", True, frame0=frame0)
    assert t.last_camera_rays()
    many = _frame(t, f"sets-{frame0}-8x1", True, calls=SPP, frame0=frame0)
    _same(many, one, f"sets-{frame0}: 8 calls of 1 sample equal 1 call of 8")
    acc, rng = np.zeros((H, W, 4), np.float32), host.fill_rng(SEED, W, H)
    t.reset_stats()
    for smp in range(SPP):
        k = (frame0 + smp) % 2
        if k:       # the state of pixel p goes to pixel pi(p), whose camera ray p takes
            acc, rng = _permute(acc, inv), _permute(rng, inv)
        acc, rng, st = _frame(t, f"sets-{frame0}-ref", False, spp=1, frame0=frame0 + smp, rng=rng, accum=acc, reset=False)
        if k:
            acc, rng = _permute(acc, PI), _permute(rng, PI)
    _same(one, (acc, rng, st), f"sets-{frame0}")


# ---------------------------------------------------------------------- 4. a panorama lit by its map
def test_an_equirectangular_set_is_lit_where_its_rays_leave_the_scene(rgpu):
    """The eye of light_oracle_cases.replay_camera stands outside Cornell's open side: a panorama from there sees the box and the sky.
    The map is the "sun" map plus a floor of 0.05, so no texel is black: a ray that leaves the scene carries radiance whatever it meets."""
    t, s = rgpu, lc.cornell("mem", False, False)
    _upload(t, s, cam=lc.replay_camera(W, H), env=None)
    sky = np.ascontiguousarray(lc.env_map("sun") + np.float32(0.05))
    assert (sky > 0).all()
    try:
        t.set_environment_map(sky)
        t.generate_camera_rays(abi.RAYS_EQUIRECT, 2, host.halton_offsets(2))
        hits = t.trace_rays(np.ascontiguousarray(t.download_camera_rays(0).ravel()), production=True)
    except TracerError:
        FAULTED.append("equirect-setup")
        raise
    miss = (hits["hit"] == 0).reshape(H, W)
    print(f"equirect: {int(miss.sum())} of {N} set-0 rays miss")
    assert miss.any() and (~miss).any()
    acc, _, st = _frame(t, "equirect", True)
    assert t.last_camera_rays() and t.last_kernel()["variant"] == "env"
    assert np.isfinite(acc).all() and st[1] == N * SPP
    assert (acc[..., :3][miss] > 0).any(axis=-1).all()


# ---------------------------------------------------------------------- 5. refusals
def _refused(fn, status):
    with pytest.raises(TracerError) as e:
        fn()
    assert e.value.status == status, e.value


def test_refusals_are_the_union_of_the_two_flags(rgpu):
    t, s = rgpu, lc.cornell("lds", False, False)
    _upload(t, s)
    t.seed(SEED); t.clear_accum()
    before = t.download_accum(), t.download_rng()
    pair = lambda **kw: t.render(**{**dict(spp=SPP, integrator=lc.MIS, camera_rays=True, env_light=True), **kw})
    _refused(pair, abi.ERR_UNSUPPORTED)                                                      # no rays in force
    t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
    _refused(lambda: pair(integrator=lc.PATH), abi.ERR_UNSUPPORTED)                          # tracePath
    _refused(lambda: pair(integrator=lc.VOLUME), abi.ERR_UNSUPPORTED)
    _refused(lambda: pair(mesh_lights=True), abi.ERR_UNSUPPORTED)                            # with TRC_FLAG_MESH_LIGHTS added
    _refused(lambda: pair(view_height=15), abi.ERR_UNSUPPORTED)                              # a stacked view
    for kw in (dict(sobol=True), dict(collect_stats=True)):
        _refused(lambda: pair(**kw), abi.ERR_UNSUPPORTED)
    t.set_environment_map(None)
    _refused(pair, abi.ERR_UNSUPPORTED)                                                      # no map
    assert np.array_equal(u32(t.download_accum()), u32(before[0])) and np.array_equal(t.download_rng(), before[1])
    try:                                                                                     # ... and with the map back the pair runs
        t.set_environment_map(lc.env_map("sun"))
        pair()
        assert t.last_camera_rays() and t.last_kernel()["variant"] == "env"
        assert (u32(t.download_accum()) != u32(before[0])).any()
    except TracerError:
        FAULTED.append("refusals")
        raise


# ---------------------------------------------------------------------- 6. a tile mask and trc_render_adaptive
def test_tile_mask_and_adaptive_passes(rgpu):
    t, s = rgpu, lc.cornell("mem", False, False)
    whole = _env_plain(t, "mem")                        # the pair under the camera's own rays is this frame (test 1)
    _upload(t, s)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
    rows, cols = t.tile_grid()
    mask = (np.add.outer(np.arange(rows), np.arange(cols)) % 2 == 0)
    ys, xs = np.mgrid[0:H, 0:W] // abi.TRC_TILE
    kept = mask[ys, xs]
    try:
        full = _frame(t, "mask-whole", True)
        _same(full, whole, "the whole-frame launch of the pair")
        t.set_tile_mask(mask)
        acc, rng, st = _frame(t, "mask", True)
        assert t.last_camera_rays() and t.last_kernel()["variant"] == "env"
        t.set_tile_mask(None)
    except TracerError:
        FAULTED.append("mask")
        raise
    assert 0 < kept.sum() < N and st[1] == kept.sum() * SPP
    assert np.array_equal(acc[kept].view(np.uint32), full[0][kept].view(np.uint32)) and np.array_equal(rng[kept], full[1][kept])
    assert not acc[~kept].view(np.uint32).any() and np.array_equal(rng[~kept], host.fill_rng(SEED, W, H)[~kept])
    # trc_render_adaptive with both flags in p->flags: passes of 8, 8 and 16 samples, so a tile stops at n_t = 16 or 32 and its pixels
    # hold the bits of a whole-frame launch of n_t samples
    try:
        want = {n: _frame(t, f"adaptive-whole-{n}", True, spp=n) for n in (16, 32)}
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        rep = t.render_adaptive(threshold=0.05, max_spp=32, spp=8, integrator=lc.MIS, flags=abi.FLAG_CAMERA_RAYS | abi.FLAG_ENV_LIGHT)
        assert t.last_camera_rays() and t.last_kernel()["variant"] == "env"
        paths, n_t = t.stats().paths, t.tile_samples()[ys, xs]
        acc, rng = t.download_accum(), t.download_rng()
    except TracerError:
        FAULTED.append("adaptive")
        raise
    print(f"adaptive: {rep.as_dict()}, paths {paths}, pixels at 16 / 32 samples: {int((n_t == 16).sum())} / {int((n_t == 32).sum())}")
    assert rep.passes >= 2 and rep.samples == paths == int(n_t.sum()) and np.isin(n_t, (16, 32)).all()
    for n in (16, 32):
        at = n_t == n
        assert np.array_equal(acc[at].view(np.uint32), want[n][0][at].view(np.uint32)) and np.array_equal(rng[at], want[n][1][at]), n
