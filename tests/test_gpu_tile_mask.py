"""trc_set_tile_mask on the GPU (include/tracer_abi.h): a masked trc_render leaves every pixel outside the mask bit for bit alone and gives
the pixels inside the bits of an unmasked render, for every launch shape; what the context knows about block costs survives a mask that
only clears tiles; refusals change nothing.  40 x 36 frames: 3 x 3 tiles with a partial tile column 8 wide and a partial tile row 4 high,
and a partial row of 8 x 8 blocks.  Every test opens its own context, so no mask leaks into another file's tests."""
import numpy as np
import pytest

import adaptive_ref as ar
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
W, H, SEED = 40, 36, 9
PATH, MIS = abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS
TH, TW = ar.tile_grid(W, H)
CHECKER = np.array([[(x + y) % 2 == 0 for x in range(TW)] for y in range(TH)], dtype=np.uint8)
ROWS = [np.repeat(np.arange(TH)[:, None] == r, TW, axis=1).astype(np.uint8) for r in range(TH)]
EMPTY = np.zeros((TH, TW), dtype=np.uint8)

_SCENES, _PLAIN = {}, {}


def scene(kind):
    """'spheres': Cornell + spheres; 'lds': Cornell + a 48-triangle ball (the whole tree is staged in LDS); 'mem': Cornell + a 5 000-triangle
    ball (read from memory) -- the two residences of tests/test_gpu_update_vertices.py"""
    if kind not in _SCENES:
        _SCENES[kind] = (host.HostScene(abi.SCENE_CORNELL_SPHERES) if kind == "spheres" else
                         host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1) if kind == "lds" else host.Mesh.ball(50, 50, 0.08)))
    return _SCENES[kind]


def setup(t, kind, knobs=()):
    t.upload_scene(scene(kind).view); t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    for name, value in knobs:
        t.debug_set(name, value)


def start(t):
    t.seed(SEED); t.clear_accum(); t.reset_stats()


def render(t, spp, integrator, kw):
    """`spp` samples: launches of fewer than 8 as calls of one sample each, which the library keeps and coalesces"""
    if spp < 8:
        for k in range(spp):
            t.render(spp=1, integrator=integrator, frame0=k, **kw)
    else:
        t.render(spp=spp, integrator=integrator, **kw)


def planes(t):
    acc, rng, st = t.download_accum().view(np.uint32), t.download_rng(), t.stats()
    return acc, rng, st.rays, st.paths


def plain(kind, spp, integrator, kw=(), knobs=()):
    """the unmasked render of a second context, made once -> (accumulator bits, RNG, rays, paths, cleared accumulator bits, seeded RNG)"""
    key = (kind, spp, integrator, tuple(kw), tuple(knobs))
    if key not in _PLAIN:
        with Tracer(0) as ref:
            setup(ref, kind, knobs)
            start(ref)
            cleared, seeded = ref.download_accum().view(np.uint32), ref.download_rng()
            render(ref, spp, integrator, dict(kw))
            _PLAIN[key] = planes(ref) + (cleared, seeded)
    return _PLAIN[key]


def pixel_mask(mask):
    return np.repeat(np.repeat(np.asarray(mask) != 0, ar.TILE, axis=0), ar.TILE, axis=1)[:H, :W]


CASES = [("spheres", spp, PATH, (), ()) for spp in (1, 4, 8, 16, 40)] + [
    ("spheres", 16, MIS, (), ()),
    ("spheres", 4, PATH, (), (("strip_force", 2),)),                    # strips
    ("spheres", 3, MIS, (), (("strip_force", 3),)),
    ("spheres", 16, PATH, (("tile_nranks", 2), ("tile_rank", 1)), ()),
    ("spheres", 16, MIS, (("tile_nranks", 2), ("tile_rank", 0)), ()),
    ("spheres", 16, PATH, (("small_blocks", True),), ()),              # 4 x 4 blocks
    ("spheres", 16, PATH, (("view_height", 18),), ()),                 # two stacked views
    ("spheres", 8, PATH, (("collect_stats", True),), ()),              # an instrumented launch
    ("lds", 16, PATH, (), ()), ("lds", 8, MIS, (), ()),
    ("mem", 16, PATH, (), ()), ("mem", 8, MIS, (), ()),                 # persistent workgroups
    ("mem", 16, PATH, (), (("no_pwg", 1),)),
]


@pytest.mark.parametrize("kind,spp,integrator,kw,knobs", CASES)
def test_masked_renders(kind, spp, integrator, kw, knobs):
    """a checkerboard and its complement, every tile row alone, the empty mask, and no mask again: one context, mask after mask"""
    acc_ref, rng_ref, rays_ref, paths_ref, cleared, seeded = plain(kind, spp, integrator, kw, knobs)
    assert acc_ref.any() and not cleared.any()
    with Tracer(0) as t:
        setup(t, kind, knobs)
        rays = {}
        for name, mask in [("checker", CHECKER), ("rest", 1 - CHECKER)] + [(f"row{r}", m) for r, m in enumerate(ROWS)] + [("empty", EMPTY), ("none", None)]:
            start(t)
            t.set_tile_mask(mask)
            assert np.array_equal(t.tile_mask(), np.ones((TH, TW), np.uint8) if mask is None else mask)
            render(t, spp, integrator, dict(kw))
            acc, rng, rays[name], paths = planes(t)
            on = pixel_mask(np.ones((TH, TW)) if mask is None else mask)[..., None]
            assert np.array_equal(acc, np.where(on, acc_ref, cleared)), name
            assert np.array_equal(rng, np.where(on, rng_ref, seeded)), name
            touched = int((np.where(on, rng_ref, seeded) != seeded).any(axis=2).sum())      # pixels of the mask that this rank owns
            assert paths == touched * spp, name
        assert rays["checker"] + rays["rest"] == rays_ref == rays["none"] and sum(rays[f"row{r}"] for r in range(TH)) == rays_ref
        # (two ranks own the tiles checkerboard-wise themselves: there the checkerboard is the whole share or none of it, the rows split it)
        assert rays["empty"] == 0 and (0 < rays["checker"] < rays_ref or dict(kw).get("tile_nranks", 1) > 1) and 0 < rays["row1"] < rays_ref


def test_a_mask_change_flushes_the_kept_launch_under_the_old_mask():
    acc_ref, rng_ref, _, _, cleared, seeded = plain("spheres", 1, PATH)
    with Tracer(0) as t:
        setup(t, "spheres")
        start(t)
        t.set_tile_mask(CHECKER)
        t.render(spp=1, integrator=PATH)             # kept for coalescing
        t.set_tile_mask(None)                        # ... and launched here, under the checkerboard
        acc, rng, _, paths = planes(t)
        on = pixel_mask(CHECKER)[..., None]
        assert np.array_equal(acc, np.where(on, acc_ref, cleared)) and np.array_equal(rng, np.where(on, rng_ref, seeded))
        assert paths == int(on.sum())


def test_resize_drops_the_mask():
    acc_ref = plain("spheres", 8, PATH)[0]
    with Tracer(0) as t:
        setup(t, "spheres")
        t.set_tile_mask(EMPTY)
        t.resize(W, H)
        assert t.tile_mask().all()
        start(t); t.render(spp=8, integrator=PATH)
        assert np.array_equal(t.download_accum().view(np.uint32), acc_ref)


def test_sppm_ignores_the_mask():
    frames = []
    for mask in (None, EMPTY):
        with Tracer(0) as t:
            setup(t, "spheres")
            t.set_tile_mask(mask)
            t.clear_accum(); t.seed(8); t.sppm_init(9); t.sppm_frames(1)
            frames.append(t.download_accum().view(np.uint32))
    assert frames[0].any() and np.array_equal(frames[0], frames[1])


# --------------------------------------------------------------------------------------------------- carried costs
CLEARED = (0, 4, 8)                   # a full tile, the middle one, the 8 x 4 corner


def settled(t, integrator, knobs=()):
    setup(t, "spheres", knobs)
    for _ in range(3):
        start(t); t.render(spp=16, integrator=integrator)
    return t.block_costs()


def as_dict(tiles, costs):
    return {int(b): int(c) for b, c in zip(tiles, costs)}


def kept_blocks(tiles, mask):
    """the 8 x 8 blocks (x | y << 16) of `tiles` whose tile the mask keeps"""
    return [int(b) for b in tiles if mask.ravel()[((int(b) >> 16) * 8 // ar.TILE) * TW + (int(b) & 0xFFFF) * 8 // ar.TILE]]


@pytest.mark.parametrize("forget", [0, 1])
def test_costs_across_a_mask_that_only_clears_tiles(forget):
    """After settled 16-sample launches, a mask that clears three tiles leaves the costs of the surviving blocks -- every block whole here
    (knob no_split), so a block's cost as one block is its entry -- as they were, in the new list's order, and the next launch is ONE
    launch; with knob mask_forgets_costs it is a cold head + the rest.  The frame is the same either way."""
    mask = np.ones((TH, TW), np.uint8); mask.ravel()[list(CLEARED)] = 0
    acc_ref, rng_ref, _, _, cleared, seeded = plain("spheres", 16, MIS)
    with Tracer(0, hooks=True) as t:
        tiles, costs, shift = settled(t, MIS, (("no_split", 1), ("mask_forgets_costs", forget)))
        assert shift == 3 and len(tiles) == 25 and (costs > 0).all() and not (costs >> 29).any()
        before = as_dict(tiles, costs)
        t.set_tile_mask(mask)
        tiles2, costs2, _ = t.block_costs()
        assert [int(b) for b in tiles2] == kept_blocks(tiles, mask) and 0 < len(tiles2) < 25
        if not forget:
            assert as_dict(tiles2, costs2) == {b: before[b] for b in kept_blocks(tiles, mask)}
        launches = t.last_kernel()["launches"]
        start(t); t.render(spp=16, integrator=MIS)
        assert t.last_kernel()["launches"] - launches == (2 if forget else 1)
        on = pixel_mask(mask)[..., None]
        assert np.array_equal(t.download_accum().view(np.uint32), np.where(on, acc_ref, cleared))
        assert np.array_equal(t.download_rng(), np.where(on, rng_ref, seeded))
        # a mask that sets a tile again is a new list: its first launch measures afresh
        t.set_tile_mask(None)
        launches = t.last_kernel()["launches"]
        start(t); t.render(spp=16, integrator=MIS)
        assert t.last_kernel()["launches"] - launches == 2
        assert np.array_equal(t.download_accum().view(np.uint32), acc_ref)


def test_costs_of_blocks_that_ran_in_parts_are_carried_as_one_block():
    """tracePath on 25 blocks runs them as quarters: what is carried is each block's cost as ONE block -- no part flags, nothing zero -- and
    two masks in a row, each a subset of the one before, still leave one launch"""
    mask = np.ones((TH, TW), np.uint8); mask.ravel()[list(CLEARED)] = 0
    smaller = mask.copy(); smaller.ravel()[1] = 0
    acc_ref, _, _, _, cleared, _ = plain("spheres", 16, PATH)
    with Tracer(0, hooks=True) as t:
        tiles, costs, _ = settled(t, PATH)
        assert (costs >> 31).any()                            # some block ran in parts
        t.set_tile_mask(mask)
        t.set_tile_mask(smaller)
        tiles2, costs2, _ = t.block_costs()
        assert [int(b) for b in tiles2] == kept_blocks(tiles, smaller)
        assert (costs2 > 0).all() and not (costs2 >> 29).any()
        launches = t.last_kernel()["launches"]
        start(t); t.render(spp=16, integrator=PATH)
        assert t.last_kernel()["launches"] - launches == 1
        assert np.array_equal(t.download_accum().view(np.uint32), np.where(pixel_mask(smaller)[..., None], acc_ref, cleared))


# --------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing():
    from tracer_amd.gloo_collectives import ALLGATHER_FN, ALLREDUCE_FN, REDUCE_FN, Collectives

    class Table:                     # a one-rank group whose collectives are never called
        def __init__(self):
            self.cb = (REDUCE_FN(lambda *a: 0), ALLREDUCE_FN(lambda *a: 0), ALLGATHER_FN(lambda *a: 0))
            self.table = Collectives(None, 0, 0, *self.cb)

    acc_ref, rng_ref, _, _, cleared, seeded = plain("spheres", 8, PATH)
    on = pixel_mask(CHECKER)[..., None]
    with Tracer(0) as t:
        with pytest.raises(TracerError) as e:             # no frame yet
            t.set_tile_mask(None)
        assert e.value.status == abi.ERR_NO_FRAME
        setup(t, "spheres")
        t.set_tile_mask(CHECKER)
        for n in (0, TH * TW - 1, TH * TW + 1, W * H):
            with pytest.raises(TracerError) as e:
                t.set_tile_mask(np.ones(TH * TW, np.uint8), n_tiles=n)
            assert e.value.status == abi.ERR_INVALID_ARG
        t.set_collectives(Table(), 1, 0)
        for call in (lambda: t.set_tile_mask(None), lambda: t.set_tile_mask(EMPTY), t.tile_snapshot, t.tile_error, t.tile_errors):
            with pytest.raises(TracerError) as e:
                call()
            assert e.value.status == abi.ERR_UNSUPPORTED
        t.group_finalize()
        assert np.array_equal(t.tile_mask(), CHECKER)
        start(t); t.render(spp=8, integrator=PATH)
        assert np.array_equal(t.download_accum().view(np.uint32), np.where(on, acc_ref, cleared))
        assert np.array_equal(t.download_rng(), np.where(on, rng_ref, seeded))
