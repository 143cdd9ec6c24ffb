"""trc_denoise_guide_rays (include/tracer_abi.h "A denoiser that follows the rays"): with the switch on, the SVGF G-buffer is walked along
set 0 of the context's camera-ray sets instead of along the camera's own pinhole ray.

Held to what already stands: with the camera's own rays as set 0 the switch changes no bit of any plane (1); for any other set the
G-buffer is trc_trace_rays' production walk of the downloaded set, texel by texel (2); the temporal pass takes the one tap (x, y), restated
here in numpy (3); the history is dropped by a new generation of rays and by the switch, and kept across trc_set_camera (4); with motion
tracking a moved pixel has no valid history and the others keep theirs (5); refusals (6).

Scenes of tests/light_oracle_cases.py: Cornell + the 48-triangle ball (the tree in LDS) or the 1104-triangle one (read from memory),
61 x 45, traceMIS under a constant environment that is not black.  The scene's own camera sees the box through its open side with sky
around it; FAR_CAMERA stands outside and has a focus plane wide enough for an orthographic set to see the box and the sky beside it.
Everything is compared as uint32.  After a call that left an error behind nothing more of this module runs on the GPU."""
import contextlib

import numpy as np
import pytest

import light_oracle_cases as lc
import pose_ref as pr
import refit_ref as rr
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError
from tracer_amd.dtypes import GBUFFER_DTYPE

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SEED, SPP = lc.W, lc.H, lc.SEED, 8
N = W * H
FAULTED = []
PI = np.random.default_rng(31).permutation(N)


def far_camera():
    """the eye of light_oracle_cases.replay_camera with the focus plane 900 away: horizontal and vertical span the whole box"""
    return host.make_camera((500.0, 40.0, -450.0), (200.0, 450.0, 250.0), (0.0, 1.0, 0.0), 0.0, W / H, float(np.deg2rad(50.0)), 900.0)


@pytest.fixture
def t():
    """a context of its own with the test hooks (the switch is context state)"""
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    with Tracer(0, hooks=True) as trc:
        yield trc


@contextlib.contextmanager
def guard(what):
    try:
        yield
    except TracerError:
        FAULTED.append(what)
        raise


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def setup(t, s, cam=None):
    t.upload_scene(s.view); t.upload_triangle_materials(s.tri); t.upload_textures(s.images)
    t.set_camera(cam if cam is not None else s.cam); t.set_environment(lc.ENV_RGB); t.set_environment_map(None); t.resize(W, H)
    t.seed(SEED); t.clear_accum()


def step(t, k, p=None, flagged=False):
    """SPP more samples on the accumulator, then trc_denoise"""
    t.render(spp=SPP, frame0=SPP * k, integrator=lc.MIS, camera_rays=flagged)
    t.denoise(p)


def planes(t):
    return dict(gbuffer=t.download_gbuffer().view(np.uint32), out=bits(t.download_denoised()), n=bits(t.download_history_length()),
                **{k: bits(v) for k, v in zip(("integrated", "history", "moments"), t.denoise_state())})


def keeps(g):
    """the pixels whose one tap (x, y) finds the pixel's own surface again: a hit whose G-buffer normal passes step 2's normal test against
    itself, (n.x n.x + n.y n.y) + n.z n.z >= 0.9 in binary32.  The interpolated shading normal of a ball's facet is not normalised: measured
    with the oracle's walk, 135 of the 2318 hits of the 48-triangle ball's scene under its own camera have a shorter one (squared length
    down to 0.70), 97 of 2318 with the 1104-triangle ball (down to 0.10 at its poles).  Such a pixel has n = 1 in every frame, with the
    switch off as with it on: step 2 as the header states it.  So "history length k on hits" is asserted on these pixels, and n = 1 on the rest."""
    n = g["normal"]
    return (g["id"] != abi.GBUFFER_MISS) & ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2] >= F(0.9))


def make_set(t, s, kind):
    """set 0 of a kind: generated from the camera in force, or the host's pinhole rays permuted"""
    if kind == "permuted":
        t.upload_camera_rays(np.ascontiguousarray(host.generate_camera_rays(s.cam, W, H)[0].ravel()[PI].reshape(H, W)))
    else:
        t.generate_camera_rays({"ortho": abi.RAYS_ORTHOGRAPHIC, "equirect": abi.RAYS_EQUIRECT, "pinhole": abi.RAYS_PINHOLE}[kind], 1, None)


def camera_of(s, kind):
    return None if kind in ("permuted", "pinhole") else far_camera()


def production_hits(t):
    hits = t.trace_rays(np.ascontiguousarray(t.download_camera_rays(0).ravel()), production=True).reshape(H, W)
    hit = hits["hit"] != 0
    assert hit.any() and (~hit).any()
    return hits, hit


# ---------------------------------------------------------------------- 1. the camera's own rays: the switch changes nothing
@pytest.mark.parametrize("demodulate", (False, True), ids=("plain", "demodulate"))
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_own_pinhole_rays_switch_on_equals_switch_off(t, residence, demodulate):
    s = lc.cornell(residence, False, True)
    runs = {}
    with guard(f"own-{residence}-{demodulate}"):
        for on in (False, True):
            setup(t, s)
            t.denoise_guide_rays(on)
            t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
            p = t.denoise_params(demodulate=demodulate)
            runs[on] = []
            for k in range(3):
                step(t, k, p)
                runs[on].append(planes(t))
    for k in range(3):
        for name, want in runs[False][k].items():
            bad = int((runs[True][k][name] != want).sum())
            print(f"{residence} demodulate={demodulate} call {k} {name}: {bad} words differ")
            assert bad == 0, (k, name)
    g = runs[True][2]["gbuffer"].view(GBUFFER_DTYPE).reshape(H, W)
    hit, kept = g["id"] != abi.GBUFFER_MISS, keeps(g)
    n = runs[True][2]["n"].view(F).reshape(H, W)
    print(f"{residence}: {int(hit.sum())} hits, {int(kept.sum())} of them keep their history")
    assert kept.sum() > hit.sum() * 0.9 and (~hit).any() and (n[kept] == 3).all() and (n[~kept] == 1).all()   # the one tap under an unchanged camera, either way


# ---------------------------------------------------------------------- 2. other sets: the G-buffer is trc_trace_rays of set 0
@pytest.mark.parametrize("kind", ("ortho", "equirect", "permuted"))
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_gbuffer_is_the_production_walk_of_set_0(t, residence, kind):
    s = lc.cornell(residence, False, True)
    with guard(f"gbuffer-{residence}-{kind}"):
        setup(t, s, camera_of(s, kind))
        step(t, 0)
        g_off = t.download_gbuffer()                                # the camera's own G-buffer (switch off)
        t.denoise_guide_rays(True)
        make_set(t, s, kind)
        hits, hit = production_hits(t)
        step(t, 1, flagged=True)
        g = t.download_gbuffer()
    print(f"{residence} {kind}: {int(hit.sum())} hits, {int((~hit).sum())} misses")
    assert np.array_equal(g["id"] != abi.GBUFFER_MISS, hit)
    assert np.array_equal(bits(g["depth"][hit]), bits(hits["t"][hit])) and np.array_equal(bits(g["normal"][hit]), bits(hits["sn"][hit]))
    assert np.array_equal(g["id"][hit], hits["material"][hit])
    miss = g[~hit]
    assert (miss["depth"] == np.inf).all() and not bits(miss["normal"]).any() and (miss["albedo"] == 1.0).all()
    if kind == "permuted":                                          # the whole texel, albedo included
        assert np.array_equal(g.view(np.uint32).reshape(N, 8), g_off.view(np.uint32).reshape(N, 8)[PI])
        assert (g.view(np.uint32) != g_off.view(np.uint32)).any()
    else:
        assert (bits(g["depth"]) != bits(g_off["depth"])).any()     # another projection is another G-buffer


# ---------------------------------------------------------------------- 3. the one-tap blend, restated
def test_the_one_tap_blend(t):
    """iterations = 0, no demodulation: the integrated colour is step 2's blend alone.  sw = 1 and the sums are the tap's own values, so
    pc = history, n = n' + 1, a = max(1 / n, alpha_color), colour = pc + (c - pc) * a, every operation binary32."""
    s = lc.cornell("mem", False, True)
    with guard("blend"):
        setup(t, s, far_camera())
        t.denoise_guide_rays(True)
        make_set(t, s, "ortho")
        _, hit = production_hits(t)
        p = t.denoise_params(iterations=0)
        alpha = F(p.alpha_color)
        hist, n = None, None
        for k in range(1, 4):
            step(t, k - 1, p, flagged=True)
            c = t.download_accum()[..., :3]
            got, got_n = t.denoise_state()[0][..., :3], t.download_history_length()
            valid = keeps(t.download_gbuffer())
            assert not (valid & ~hit).any() and valid.sum() > hit.sum() * 0.9
            if hist is None:
                want, n = c.copy(), np.ones((H, W), F)
            else:
                n = np.where(valid, np.minimum(n + F(1), F(64)), F(1)).astype(F)
                a = np.maximum(F(1) / n, alpha).astype(F)[..., None]
                want = np.where(valid[..., None], (hist + ((c - hist).astype(F) * a).astype(F)).astype(F), c)
            assert (got_n[valid] == k).all() and (got_n[~valid] == 1).all(), k
            bad = int((bits(got) != bits(want)).sum())
            print(f"call {k}: {bad} words of the integrated colour differ from the restatement")
            assert bad == 0, k
            hist = want


# ---------------------------------------------------------------------- 4. what drops and what keeps the history
def test_what_drops_and_what_keeps_the_history(t):
    s = lc.cornell("mem", False, True)
    with guard("history"):
        setup(t, s, far_camera())
        t.denoise_guide_rays(True)
        make_set(t, s, "ortho")
        _, hit = production_hits(t)
        length = lambda: t.download_history_length()
        step(t, 0); step(t, 1)
        hit = keeps(t.download_gbuffer())                           # (the hits whose tap finds them again: keeps)
        assert hit.any() and (length()[hit] == 2).all()
        make_set(t, s, "ortho")                                     # the same arguments: the same bits, another generation
        step(t, 2)
        assert (length() == 1).all()
        step(t, 3)
        g = t.download_gbuffer()
        assert (length()[hit] == 2).all()
        t.set_camera(s.cam)                                         # another camera: the rays hold their own
        step(t, 4)
        assert (length()[hit] == 3).all() and (length()[~hit] == 1).all()
        assert np.array_equal(t.download_gbuffer().view(np.uint32), g.view(np.uint32))
        t.denoise_guide_rays(True)                                  # the value it has: nothing happens
        step(t, 5)
        assert (length()[hit] == 4).all()
        t.denoise_guide_rays(False)                                 # a change drops the history; the G-buffer is the camera's again
        step(t, 6)
        assert (length() == 1).all()
        assert (t.download_gbuffer().view(np.uint32) != g.view(np.uint32)).any()
        t.denoise_guide_rays(True)
        step(t, 7)
        assert (length() == 1).all()
        assert np.array_equal(t.download_gbuffer().view(np.uint32), g.view(np.uint32))


# ---------------------------------------------------------------------- 5. motion
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_moved_pixels_restart_and_the_others_keep_their_history(t, residence):
    s = lc.cornell(residence, False, False)
    centre, nv = pr.box_centre(rr.vertices_of(s.view)), s.view.n_vertex
    runs = {}
    with guard(f"motion-{residence}"):
        t.denoise_track_motion(True)
        for on in (False, True):
            setup(t, s)
            t.denoise_guide_rays(on)
            t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
            step(t, 0); step(t, 1)
            before = t.download_gbuffer()
            t.pose_vertices([(0, nv, *pr.turn(centre, np.radians(5.0)))])        # the ball turns about its centre
            step(t, 2)
            runs[on] = dict(motion=t.download_motion(), n=t.download_history_length(), g=t.download_gbuffer(), before=before)
    on, off = runs[True], runs[False]
    assert np.array_equal(on["motion"].view(np.uint32), off["motion"].view(np.uint32))      # the camera's own rays: the plane of the switch-off run
    assert np.array_equal(on["g"].view(np.uint32), off["g"].view(np.uint32))
    moved = on["motion"]["moved"] == 1
    # had history: the pixel shows, along the same ray, the surface it showed before (same id, same depth bits)
    still = ~moved & keeps(on["g"]) & (on["g"]["id"] == on["before"]["id"]) & (bits(on["g"]["depth"]) == bits(on["before"]["depth"]))
    print(f"{residence}: {int(moved.sum())} moved pixels, {int(still.sum())} still ones with history; switch off keeps {int((off['n'][moved] > 1).sum())} of the moved")
    assert moved.any() and still.any()
    assert (on["n"][moved] == 1).all()
    assert (on["n"][still] == 3).all()


# ---------------------------------------------------------------------- 6. refusals
def test_refusals(t):
    """The switch on and no rays in force: TRC_ERR_UNSUPPORTED, and nothing of the denoiser's state is touched -- the planes of the last
    trc_denoise still answer.  Rays can only come back through a call that begins a new generation, so the next accepted call starts at
    n = 1 (rule 3) and counts on from there."""
    s = lc.cornell("lds", False, True)

    def refused():
        with pytest.raises(TracerError) as e:
            t.denoise()
        assert e.value.status == abi.ERR_UNSUPPORTED, e.value

    assert t._L.trc_denoise_guide_rays(None, 1) == abi.ERR_INVALID_ARG
    with guard("refusals"):
        setup(t, s)
        t.denoise_guide_rays(True)
        refused()                                                   # before any rays
        t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
        _, hit = production_hits(t)
        step(t, 0); step(t, 1)
        kept = planes(t)
        hit = keeps(t.download_gbuffer())                           # (the coarse ball: not every hit finds itself again)
        assert hit.any() and (kept["n"].view(F).reshape(H, W)[hit] == 2).all()
        t.clear_camera_rays()
        refused()
        for name, want in planes(t).items():                        # the history survives the refused call
            assert np.array_equal(want, kept[name]), name
        t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
        step(t, 2)
        assert (t.download_history_length() == 1).all()
        step(t, 3)
        assert (t.download_history_length()[hit] == 2).all()
        t.resize(W, H)                                              # the rays go with the frame; the switch stays
        refused()
        t.seed(SEED); t.clear_accum()
        t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
        step(t, 0)
        assert (t.download_history_length() == 1).all()
        t.denoise_guide_rays(False)
        step(t, 1)                                                  # switch off: no rays needed
        t.clear_camera_rays()
        step(t, 2)
        assert (t.download_history_length()[hit] == 2).all()
