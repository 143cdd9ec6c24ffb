"""trc_tile_snapshot / trc_tile_error / trc_render_adaptive on the GPU against their restatement (tests/adaptive_ref.py), bit for bit: the
estimate on rendered and on uploaded accumulators, and the driver against the restatement's loop over PLAIN renders -- a tile that
stopped at n_t samples holds exactly the pixels and RNG texels of a plain trc_render of n_t samples.  40 x 36 frames, seed 9, Cornell +
spheres.  Every test opens its own context."""
import numpy as np
import pytest

import adaptive_ref as ar
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SEED = 40, 36, 9
PATH, MIS = abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS
TH, TW = ar.tile_grid(W, H)
H0, MAX_SPP = 8, 64

_SCENE, _PLAIN = [], {}


def setup(t):
    if not _SCENE:
        _SCENE.append(host.HostScene(abi.SCENE_CORNELL_SPHERES))
    t.upload_scene(_SCENE[0].view); t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)


def start(t):
    t.seed(SEED); t.clear_accum(); t.reset_stats()


def plain(integrator, n):
    """(accumulator, RNG) of a plain n-sample trc_render, made once per (integrator, n) on a context of its own and never changed"""
    if (integrator, n) not in _PLAIN:
        with Tracer(0) as ref:
            setup(ref); start(ref)
            if n:
                ref.render(spp=n, integrator=integrator)
            acc, rng = ref.download_accum(), ref.download_rng()
            acc.setflags(write=False); rng.setflags(write=False)
            _PLAIN[integrator, n] = (acc, rng)
    return _PLAIN[integrator, n]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def first_check(integrator):
    """E_t of every tile at n = 16 with A at 8, from plain renders and the restatement"""
    return ar.tile_errors(plain(integrator, 16)[0], plain(integrator, 8)[0])


# --------------------------------------------------------------------------------------------------- the estimate
@pytest.mark.parametrize("integrator", [MIS, PATH])
def test_estimate_after_8_plus_8_samples(integrator):
    with Tracer(0) as t:
        setup(t); start(t)
        assert not t.tile_errors().any()                              # 0 until a tile's first estimate
        t.render(spp=8, integrator=integrator)
        t.tile_snapshot()
        t.render(spp=8, integrator=integrator, frame0=8)
        t.tile_error()
        got, want = t.tile_errors(), first_check(integrator)
        print("E_t", got.ravel().tolist())
        assert np.array_equal(bits(got.ravel()), bits(want)) and want.max() > 0
        assert np.array_equal(bits(t.download_accum()), bits(plain(integrator, 16)[0]))      # the estimate reads, it does not write
        # without snapshot_after A is still the 8-sample frame: the same call gives the same answer
        t.tile_error()
        assert np.array_equal(bits(t.tile_errors().ravel()), bits(want))
        # snapshot_after: A := the accumulator, so the next estimate of an unchanged frame is 0
        t.tile_error(snapshot_after=True)
        assert np.array_equal(bits(t.tile_errors().ravel()), bits(want))
        t.tile_error()
        assert not t.tile_errors().any()
        # ... and after 16 more samples it is the estimate of (32, 16)
        t.render(spp=16, integrator=integrator, frame0=16)
        t.tile_error()
        assert np.array_equal(bits(t.tile_errors().ravel()), bits(ar.tile_errors(plain(integrator, 32)[0], plain(integrator, 16)[0])))


def test_estimate_under_a_mask_leaves_the_other_tiles_alone():
    mask = np.zeros((TH, TW), np.uint8); mask.ravel()[[1, 5, 8]] = 1
    with Tracer(0) as t:
        setup(t); start(t)
        t.render(spp=8, integrator=MIS); t.tile_snapshot(); t.render(spp=8, integrator=MIS, frame0=8)
        t.tile_error()
        first = t.tile_errors().ravel()
        t.set_tile_mask(mask)
        t.render(spp=16, integrator=MIS, frame0=16)                   # the three tiles go on to 32 samples
        acc = t.download_accum()
        t.tile_error(snapshot_after=True)
        want = ar.tile_errors(acc, plain(MIS, 8)[0], mask, first)
        got = t.tile_errors().ravel()
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got[mask.ravel() == 0]), bits(first[mask.ravel() == 0])) and (got[mask.ravel() == 1] != first[mask.ravel() == 1]).all()
        # snapshot_after wrote A on the tiles of the mask alone: with every tile in force again, those three read 0 and the rest as before
        t.set_tile_mask(None)
        t.tile_error()
        want = first.copy(); want[mask.ravel() == 1] = 0
        assert np.array_equal(bits(t.tile_errors().ravel()), bits(want))


def uploaded_planes():
    """(I, A): accumulator and snapshot planes with NaN, inf, negative, zero and sub-eps pixels and two partial tiles"""
    rs = np.random.RandomState(11)
    A = rs.gamma(0.4, 1.5, size=(H, W, 4)).astype(F)
    I = (A * rs.uniform(0.25, 1.75, size=A.shape)).astype(F)
    I[0, 0, 0] = np.nan; I[1, 17, 1] = np.inf; I[20, 3, 2] = -np.inf; A[33, 39, 0] = np.nan; A[30, 2, 1] = np.inf
    I[5, 5, :3] = 0.0; A[5, 5, :3] = 0.0                                     # black and still
    I[6, 6, :3] = 0.0                                                        # black now
    I[18, 20, :3] = (-1.0, 0.25, 0.5); I[19, 21, :3] = (-3.0, -2.0, -1.0)     # a negative channel, a negative sum
    I[16:32, 32:40, :3] = A[16:32, 32:40, :3]                                # a partial tile that did not move
    I[32:36, 0:16, :3] = 1e-6; A[32:36, 0:16, :3] = 2e-6                     # a partial tile below the eps
    return I, A


def test_estimate_on_an_uploaded_accumulator_with_nan_inf_negative_and_zero_pixels():
    I, A = uploaded_planes()
    with Tracer(0) as t:
        setup(t)
        t.upload_accum(A); t.tile_snapshot()
        t.upload_accum(I); t.tile_error(snapshot_after=True)
        got, want = t.tile_errors().ravel(), ar.tile_errors(I, A)
        print("E_t", got.tolist())
        assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all() and got[5] == 0 and got[0] > 255
        assert np.array_equal(bits(t.download_accum()), bits(I))
        # A is now I, bit for bit, NaNs included: an estimate against a third plane says so
        J = (I * F(0.5)).astype(F)
        t.upload_accum(J); t.tile_error()
        assert np.array_equal(bits(t.tile_errors().ravel()), bits(ar.tile_errors(J, I)))


# --------------------------------------------------------------------------------------------------- the driver
def check_against_the_loop(t, rep, integrator, max_spp, threshold):
    want = ar.adaptive_loop(lambda n: plain(integrator, n), W, H, H0, max_spp, threshold)
    n_t = t.tile_samples().ravel()
    print("n_t", n_t.tolist(), "E_t", t.tile_errors().ravel().tolist(), rep.as_dict())
    assert n_t.tolist() == want["n_t"].tolist()
    acc, rng = t.download_accum(), t.download_rng()
    for tile, rows, cols in ar.tile_slices(W, H):                      # every tile: a plain render of n_t samples
        ref_acc, ref_rng = plain(integrator, int(n_t[tile]))
        assert np.array_equal(bits(acc[rows, cols]), bits(ref_acc[rows, cols])), tile
        assert np.array_equal(rng[rows, cols], ref_rng[rows, cols]), tile
    assert np.array_equal(bits(acc), bits(want["accum"])) and np.array_equal(rng, want["rng"])
    assert np.array_equal(bits(t.tile_errors().ravel()), bits(want["E"]))
    assert (rep.passes, rep.active_tiles, rep.samples) == (want["passes"], want["active_tiles"], want["samples"])
    assert F(rep.max_error).view(np.uint32) == want["max_error"].view(np.uint32)
    assert rep.samples == t.stats().paths
    return want


@pytest.mark.parametrize("integrator", [MIS, PATH])
def test_driver_at_the_median_of_the_first_check(integrator):
    E16 = first_check(integrator)
    threshold = float(np.median(E16))                                  # computed here from plain renders, never a literal
    assert threshold > 0
    with Tracer(0) as t:
        setup(t); start(t)
        rep = t.render_adaptive(threshold=threshold, max_spp=MAX_SPP, spp=H0, integrator=integrator)
        want = check_against_the_loop(t, rep, integrator, MAX_SPP, threshold)
        assert np.array_equal(bits(want["first_E"]), bits(E16))
        # the driver decided something: a tile stopped at the first check and another did not
        n_t = t.tile_samples().ravel()
        assert (n_t == 16).any() and (n_t > 16).any() and ((E16 <= F(threshold)) == (n_t == 16)).all()
        assert t.tile_mask().all()                                     # no mask was set: none is left


def test_a_threshold_above_every_estimate_ends_after_two_passes():
    threshold = float(first_check(MIS).max()) * 2.0
    with Tracer(0) as t:
        setup(t); start(t)
        rep = t.render_adaptive(threshold=threshold, max_spp=MAX_SPP, spp=H0, integrator=MIS)
        check_against_the_loop(t, rep, MIS, MAX_SPP, threshold)
        assert rep.passes == 2 and rep.active_tiles == 0 and (t.tile_samples() == 16).all() and rep.samples == W * H * 16
        assert np.array_equal(bits(t.download_accum()), bits(plain(MIS, 16)[0]))


def test_a_threshold_below_every_estimate_gives_the_plain_frame():
    checks = [ar.tile_errors(plain(MIS, 2 * n)[0], plain(MIS, n)[0]) for n in (8, 16, 32)]
    threshold = float(min(c.min() for c in checks)) * 0.5
    assert threshold > 0
    with Tracer(0) as t:
        setup(t); start(t)
        rep = t.render_adaptive(threshold=threshold, max_spp=MAX_SPP, spp=H0, integrator=MIS)
        check_against_the_loop(t, rep, MIS, MAX_SPP, threshold)
        assert rep.passes == 4 and rep.active_tiles == TH * TW and rep.samples == W * H * MAX_SPP
        assert np.array_equal(bits(t.download_accum()), bits(plain(MIS, MAX_SPP)[0])) and np.array_equal(t.download_rng(), plain(MIS, MAX_SPP)[1])


def test_the_host_s_own_mask_is_restored_and_plays_no_part():
    threshold = float(np.median(first_check(MIS)))
    mine = np.zeros((TH, TW), np.uint8); mine.ravel()[[0, 7]] = 1
    with Tracer(0) as t:
        setup(t); start(t)
        t.set_tile_mask(mine)
        rep = t.render_adaptive(threshold=threshold, max_spp=MAX_SPP, spp=H0, integrator=MIS)
        check_against_the_loop(t, rep, MIS, MAX_SPP, threshold)        # the whole frame, whatever the host's mask says
        assert np.array_equal(t.tile_mask(), mine)
        start(t); t.render(spp=8, integrator=MIS)                      # ... which is in force again
        on = np.repeat(np.repeat(mine != 0, ar.TILE, axis=0), ar.TILE, axis=1)[:H, :W, None]
        assert np.array_equal(bits(t.download_accum()), np.where(on, bits(plain(MIS, 8)[0]), bits(plain(MIS, 0)[0])))


@pytest.mark.parametrize("max_spp", [40, 19])
def test_a_max_spp_that_is_no_power_of_two_times_h0_is_met_exactly(max_spp):
    threshold = float(first_check(MIS).min()) * 0.5                    # below the first check: no tile stops there
    with Tracer(0) as t:
        setup(t); start(t)
        rep = t.render_adaptive(threshold=threshold, max_spp=max_spp, spp=H0, integrator=MIS)
        want = check_against_the_loop(t, rep, MIS, max_spp, threshold)
        assert t.tile_samples().max() == max_spp and rep.passes == want["passes"] == (4 if max_spp == 40 else 3)


def test_refusals_change_nothing():
    from tracer_amd.gloo_collectives import ALLGATHER_FN, ALLREDUCE_FN, REDUCE_FN, Collectives

    class Table:                     # a one-rank group whose collectives are never called
        def __init__(self):
            self.cb = (REDUCE_FN(lambda *a: 0), ALLREDUCE_FN(lambda *a: 0), ALLGATHER_FN(lambda *a: 0))
            self.table = Collectives(None, 0, 0, *self.cb)

    mine = np.ones((TH, TW), np.uint8); mine[1, 1] = 0
    with Tracer(0) as t:
        with pytest.raises(TracerError) as e:
            t.render_adaptive(threshold=0.1, max_spp=64)
        assert e.value.status == abi.ERR_NO_SCENE
        with Tracer(0) as other:
            setup(other)                    # (makes the module's scene)
        t.upload_scene(_SCENE[0].view); t.set_camera(host.prepare_camera(W, H))
        with pytest.raises(TracerError) as e:
            t.render_adaptive(threshold=0.1, max_spp=64)
        assert e.value.status == abi.ERR_NO_FRAME
        setup(t); start(t)
        with pytest.raises(TracerError) as e:                      # no adaptive render yet
            t.tile_samples()
        assert e.value.status == abi.ERR_NO_FRAME
        t.set_tile_mask(mine)
        t.render(spp=8, integrator=MIS)
        acc, rng, paths = t.download_accum(), t.download_rng(), t.stats().paths
        bad = [dict(frame0=8), dict(spp=7), dict(spp=0), dict(max_spp=15), dict(max_spp=0), dict(threshold=0.0), dict(threshold=-0.5),
               dict(threshold=float("nan")), dict(threshold=float("inf")), dict(integrator=7), dict(tile_rank=2, tile_nranks=2)]
        for kw in bad:
            args = dict(threshold=0.1, max_spp=64, spp=8, integrator=MIS); args.update(kw)
            with pytest.raises(TracerError) as e:
                t.render_adaptive(**args)
            assert e.value.status == abi.ERR_INVALID_ARG, kw
        t.set_collectives(Table(), 1, 0)
        with pytest.raises(TracerError) as e:
            t.render_adaptive(threshold=0.1, max_spp=64, spp=8, integrator=MIS)
        assert e.value.status == abi.ERR_UNSUPPORTED
        t.group_finalize()
        assert np.array_equal(bits(t.download_accum()), bits(acc)) and np.array_equal(t.download_rng(), rng) and t.stats().paths == paths
        assert np.array_equal(t.tile_mask(), mine)
