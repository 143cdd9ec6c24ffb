"""The stages around the render kernels in libtracer_amd_fast.so: the tile mask, the per-tile error estimate, the adaptive driver and the
SVGF denoiser.  What holds in any flavour is asserted bit for bit against the fast build's OWN unmasked or plain render (bits inside a
mask, bits untouched outside it, ray sums, the composition of an adaptive frame, a constant through the denoiser); what rounds is held
to tests/fast_ref.py's float64 restatement and bound (E_t, the adaptive driver's decisions away from the threshold, a demodulated
constant), or to the exact build on robust pixels (the G-buffer).  No tolerance on the denoised picture against the exact build's."""
import numpy as np
import pytest

import adaptive_ref as ar
import fast_ref as fr
import test_gpu_adaptive as ad
import test_gpu_tile_mask as tm
from test_fast_ref_cpu import RAY_H, RAY_W, ray_view, robust
from test_gpu_adaptive import uploaded_planes
from tracer_amd import abi, host
from tracer_amd.device import Tracer

pytestmark = pytest.mark.gpu
F = np.float32
PATH, MIS = abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS


def Fast():
    return Tracer(0, fast_math=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# --------------------------------------------------------------------------------------------------- tile mask
MASK_CASES = [("spheres", 16, PATH, ()), ("mem", 8, MIS, ()), ("spheres", 4, PATH, (("strip_force", 2),))]


@pytest.mark.parametrize("kind,spp,integrator,knobs", MASK_CASES, ids=["spheres-16-path", "mem-8-mis", "spheres-4-path-strips"])
def test_masked_renders(kind, spp, integrator, knobs):
    """tests/test_gpu_tile_mask.py's loop -- a checkerboard, its complement, the empty mask, no mask -- against the fast build's own
    unmasked render"""
    with Fast() as ref:
        tm.setup(ref, kind, knobs); tm.start(ref)
        cleared, seeded = bits(ref.download_accum()), ref.download_rng()
        tm.render(ref, spp, integrator, {})
        acc_ref, rng_ref, rays_ref, _ = tm.planes(ref)
    assert acc_ref.any() and not cleared.any()
    with Fast() as t:
        tm.setup(t, kind, knobs)
        rays = {}
        for name, mask in [("checker", tm.CHECKER), ("rest", 1 - tm.CHECKER), ("empty", tm.EMPTY), ("none", None)]:
            tm.start(t)
            t.set_tile_mask(mask)
            assert np.array_equal(t.tile_mask(), np.ones((tm.TH, tm.TW), np.uint8) if mask is None else mask)
            tm.render(t, spp, integrator, {})
            acc, rng, rays[name], paths = tm.planes(t)
            on = tm.pixel_mask(np.ones((tm.TH, tm.TW)) if mask is None else mask)[..., None]
            assert np.array_equal(acc, np.where(on, acc_ref, cleared)), name                   # bits inside, untouched outside
            assert np.array_equal(rng, np.where(on, rng_ref, seeded)), name
            touched = int((np.where(on, rng_ref, seeded) != seeded).any(axis=2).sum())
            assert paths == touched * spp and (mask is None or touched == int(on.sum())), name
        assert rays["checker"] + rays["rest"] == rays_ref == rays["none"] and rays["empty"] == 0 and 0 < rays["checker"] < rays_ref


# --------------------------------------------------------------------------------------------------- tile error
def test_estimate_on_an_uploaded_accumulator_within_the_bound():
    I, A = uploaded_planes()                                                  # NaN, inf, negative, zero and sub-eps pixels, partial tiles
    assert fr.free_of_denormals(I[np.isfinite(I)], A[np.isfinite(A)])
    want = fr.tile_errors(I, A)
    with Fast() as t:
        ad.setup(t)
        t.upload_accum(A); t.tile_snapshot()
        t.upload_accum(I); t.tile_error(snapshot_after=True)
        got = t.tile_errors().ravel()
        print("E_t", got.tolist(), "bound", fr.bound(want).tolist())
        assert np.isfinite(got).all() and fr.within(got, want).all(), (got, want.v, fr.bound(want))
        assert got[5] == 0 and got[0] > 255                                   # the still tile; the tile with a NaN pixel (the cap)
        assert np.array_equal(bits(t.download_accum()), bits(I))              # the estimate reads, it does not write
        J = (I * F(0.5)).astype(F)                                            # A is now I, NaNs included
        t.upload_accum(J); t.tile_error()
        assert fr.within(t.tile_errors().ravel(), fr.tile_errors(J, I)).all()


# --------------------------------------------------------------------------------------------------- render_adaptive
_PLAIN = {}


def plain(n):
    """(accumulator, RNG) of the FAST build's plain n-sample traceMIS render of test_gpu_adaptive's frame, made once"""
    if n not in _PLAIN:
        with Fast() as ref:
            ad.setup(ref); ad.start(ref)
            ref.render(spp=n, integrator=MIS)
            _PLAIN[n] = (ref.download_accum(), ref.download_rng())
    return _PLAIN[n]


def test_adaptive_driver_decides_as_the_float64_estimate_says():
    W, H, H0, MAX = ad.W, ad.H, ad.H0, ad.MAX_SPP
    first = fr.tile_errors(plain(2 * H0)[0], plain(H0)[0])
    threshold = float(F(np.median(first.v)))                                  # from the planes, never a literal
    mine = np.zeros((ad.TH, ad.TW), np.uint8); mine.ravel()[[0, 7]] = 1
    with Fast() as t:
        ad.setup(t); ad.start(t)
        t.set_tile_mask(mine)
        rep = t.render_adaptive(threshold=threshold, max_spp=MAX, spp=H0, integrator=MIS)
        assert np.array_equal(t.tile_mask(), mine)                            # the host's mask is restored
        n_t, E_dev = t.tile_samples().ravel(), t.tile_errors().ravel()
        acc_dev, rng_dev = t.download_accum(), t.download_rng()
        paths = t.stats().paths
    # replay the loop on the fast build's own plain renders: a tile that stopped at n_t holds the pixels of render(n_t), in any flavour
    acc, A = plain(H0)[0].copy(), plain(H0)[0].copy()
    active = np.ones(ad.TH * ad.TW, bool)
    n, passes, checks, decided, judged = H0, 1, 0, 0, 0
    while n < MAX and active.any():
        n += min(n, MAX - n)
        passes += 1
        for tile, rows, cols in ar.tile_slices(W, H):
            if active[tile]:
                acc[rows, cols] = plain(n)[0][rows, cols]
        est = fr.tile_errors(acc, A)
        for tile, rows, cols in ar.tile_slices(W, H):
            if not active[tile]:
                continue
            A[rows, cols] = acc[rows, cols]
            checks += 1
            left = n_t[tile] == n and (n < MAX or E_dev[tile] <= F(threshold))      # what the device decided at this check
            if abs(est.v[tile] - threshold) > fr.bound(est)[tile]:
                assert left == (est.v[tile] <= threshold), (tile, n, est.v[tile], threshold)
                decided += 1
            if n_t[tile] == n:                                                # the tile's last estimate is the one downloaded
                assert fr.within(E_dev[tile], est[tile]), (tile, n, E_dev[tile], est.v[tile], fr.bound(est)[tile])
                judged += 1
            else:
                assert n_t[tile] > n
            active[tile] = not left
    assert judged == ad.TH * ad.TW and 2 * decided > checks                    # every tile was judged, most checks were decided by the bound
    assert (n_t == 2 * H0).any() and (n_t > 2 * H0).any()                     # the driver decided something
    assert rep.passes == passes and rep.active_tiles == int(active.sum())
    assert rep.samples == int((ar.tile_pixels(W, H) * n_t.astype(np.int64)).sum()) == paths
    for tile, rows, cols in ar.tile_slices(W, H):                             # every tile: the fast build's plain render of n_t samples
        assert np.array_equal(bits(acc_dev[rows, cols]), bits(plain(int(n_t[tile]))[0][rows, cols])), tile
        assert np.array_equal(rng_dev[rows, cols], plain(int(n_t[tile]))[1][rows, cols]), tile


# --------------------------------------------------------------------------------------------------- denoiser
def denoise_setup(t, view):
    t.upload_scene(view); t.set_camera(host.prepare_camera(RAY_W, RAY_H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(RAY_W, RAY_H)
    t.seed(3); t.clear_accum()


def test_gbuffer_is_the_exact_build_s_on_robust_pixels(gpu):
    view = ray_view("mem", "uploaded")
    ok = robust("mem", "uploaded").reshape(RAY_H, RAY_W)
    denoise_setup(gpu, view); gpu.denoise(); want = gpu.download_gbuffer()
    with Fast() as t:
        denoise_setup(t, view); t.denoise(); got = t.download_gbuffer()
    assert np.array_equal(got["id"][ok], want["id"][ok])
    assert np.array_equal(bits(got["albedo"][ok]), bits(want["albedo"][ok]))
    hit = ok & (want["id"] != 0xFFFFFFFF)
    assert hit.sum() > 0.5 * hit.size and (~(want["id"] != 0xFFFFFFFF)).any()
    assert (np.abs(got["depth"][hit].astype(np.float64) - want["depth"][hit]) <= 1e-3 * want["depth"][hit]).all()
    assert np.isinf(got["depth"][ok & ~hit]).all()


def check_history(n, g, frame):
    """history length: 1 everywhere after a reset, and on misses always; after a second trc_denoise under the same camera 2 on every hit
    pixel whose tap is consistent -- same id and depth trivially, and dot(normal, normal) >= 0.9 (step 2 of the header), which an
    interpolated normal at the ball's pole misses in the exact build too.  Pixels whose dot product is within its own bound of 0.9 are
    not judged."""
    hit = g["id"] != abi.GBUFFER_MISS
    assert (n[~hit] == 1).all()
    if frame == 1:
        assert (n[hit] == 1).all()
        return
    nn = fr.given(np.ascontiguousarray(g["normal"]))
    d = fr.add(fr.add(fr.mul(nn[..., 0], nn[..., 0]), fr.mul(nn[..., 1], nn[..., 1])), fr.mul(nn[..., 2], nn[..., 2]))
    nine = float(F(0.9))
    consistent, broken = hit & (d.v - nine > fr.bound(d)), hit & (nine - d.v > fr.bound(d))
    assert consistent.sum() > 0.99 * hit.sum()
    assert (n[consistent] == 2).all() and (n[broken] == 1).all()


def one_albedo_around(g, radius):
    """hit pixels all of whose in-bounds hit neighbours within `radius` (Chebyshev) have their albedo, bit for bit"""
    hit = g["id"] != abi.GBUFFER_MISS
    a = bits(g["albedo"])
    H, W = hit.shape
    ok = hit.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            ok[yd, xd] &= ~(hit[ys, xs] & (a[ys, xs] != a[yd, xd]).any(axis=2))
    return ok


ITERATIONS = 2                                   # a-trous steps 1 and 2: a pixel's output depends on inputs within 2 * (1 + 2) = 6 pixels


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
def test_a_constant_accumulator_through_the_denoiser(demodulate):
    """without demodulation a constant comes back bit-exact on hit pixels (the header writes the blends and sums as corrections of the
    centre value for exactly this); misses pass through.  With TRC_DENOISE_DEMODULATE the filter's input is c / albedo, which is constant
    only where the albedo is: there the constant comes back within the bound of one division and one product.  Where a material of another
    albedo lies within the filter's reach (6 pixels at two iterations) the demodulated input is a step, not a constant, and the filter
    blends across it in the exact build too: those pixels are not judged."""
    const = np.array([0.3125, 0.7, 0.123], F)
    with Fast() as t:
        denoise_setup(t, ray_view("mem", "uploaded"))
        acc = np.empty((RAY_H, RAY_W, 4), F); acc[..., :3] = const; acc[..., 3] = F(1)
        rs = np.random.RandomState(4)
        t.upload_accum(acc)
        t.denoise(demodulate=demodulate, iterations=ITERATIONS)
        g = t.download_gbuffer()
        hit = g["id"] != abi.GBUFFER_MISS
        assert hit.any() and (~hit).any()
        noisy = acc.copy(); noisy[~hit, :3] = rs.uniform(0, 2, ((~hit).sum(), 3)).astype(F)      # misses: anything, they pass through
        for frame in (1, 2):
            t.upload_accum(noisy)
            if frame == 1:
                t.denoise_reset()
            t.denoise(demodulate=demodulate, iterations=ITERATIONS)
            out = t.download_denoised()
            assert np.array_equal(bits(out[~hit]), bits(noisy[~hit])), frame
            assert np.array_equal(bits(out[..., 3]), bits(noisy[..., 3]))
            if demodulate:
                flat = one_albedo_around(g, 2 * (2 ** ITERATIONS - 1))
                assert flat.sum() > 1000 and len(np.unique(bits(g["albedo"][flat]), axis=0)) >= 3
                a = np.maximum(g["albedo"][flat], F(abi.DENOISE_ALBEDO_EPS))
                c = fr.given(np.broadcast_to(const, a.shape).copy())
                assert fr.within(out[flat][:, :3], fr.mul(fr.div(c, fr.given(a)), fr.given(a))).all(), frame
            else:
                assert np.array_equal(bits(out[hit][:, :3]), bits(np.broadcast_to(const, (int(hit.sum()), 3)))), frame
            check_history(t.download_history_length(), g, frame)


def test_denoised_render_stays_within_the_hit_pixels_range():
    with Fast() as t:
        denoise_setup(t, ray_view("mem", "uploaded"))
        t.render(spp=8, integrator=MIS)
        acc = t.download_accum()
        for frame in (1, 2):
            t.denoise()
            out = t.download_denoised()
            g = t.download_gbuffer()
            hit = g["id"] != abi.GBUFFER_MISS
            assert np.isfinite(out).all()
            assert np.array_equal(bits(out[~hit]), bits(acc[~hit]))
            for ch in range(3):
                lo, hi = float(acc[hit][:, ch].min()), float(acc[hit][:, ch].max())
                w = 2.0 ** -20 * max(abs(lo), abs(hi))
                assert lo - w <= out[hit][:, ch].min() and out[hit][:, ch].max() <= hi + w, (frame, ch)
            assert not np.array_equal(bits(out[hit]), bits(acc[hit]))
            check_history(t.download_history_length(), g, frame)
