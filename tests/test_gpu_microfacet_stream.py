"""The Metal lobe through the Beckmann lobes' instruction stream (dev_bsdf.hpp, TRC_MICROFACET_STREAM) against the form with a branch
of its own, through the device hook trc_material_s_f_test, which instantiates both whatever the render kernels were compiled with:

  * old form against new form on wi, attenuation and pdf, bit for bit (a NaN equals a NaN: microfacet_cases.same_bits), with pdf_out
    pre-filled with a sentinel that the early-outs must leave in place -- every material type alone (edge set + 2^18 seeded inputs),
    and wavefronts holding one family alone, both, and the four materials lane by lane (tests/microfacet_cases.py: layouts);
  * both forms against the oracle's Material::S_F on the edge set and the first 4096 seeded inputs of every type;
  * frames of the config-2 scene (Cornell box + 12 spheres: Metal, Plastic and Glass lanes meet in a wavefront) against the oracle on
    the three shapes of the LDS-resident tracePath kernels: k_render<true,false,0,false>, the strip kernel, k_render_dense.

After a TracerError (a device fault included) nothing more of this module is asked of the GPU."""
import numpy as np
import pytest

import microfacet_cases as mc
from oracle import pyoracle as po
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu

FAULTED = []
SEED = 0xC0FFEE
W, H = 96, 64
DENSE_W, DENSE_H, DENSE_SPP, DENSE_NRANKS = 1916, 1076, 8, 64      # the smallest class of frame k_render_dense is given (test_gpu_kernel_census.py)
_OUT = {}


@pytest.fixture(scope="module")
def mgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


@pytest.fixture(scope="module")
def layouts():
    return mc.layouts()


def _s_f(t, key, inputs, stream, pdf_init):
    """the hook's answer for one layout, computed once per (layout, form, initial pdf)"""
    k = (key, stream, float(pdf_init))
    if k not in _OUT:
        if FAULTED:
            pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
        try:
            _OUT[k] = t.material_s_f_test(*inputs, stream=stream, pdf_init=pdf_init)
        except TracerError:
            FAULTED.append(f"{key} stream={stream}")
            raise
    return _OUT[k]


def _report(name, types, wo, uu, a, b):
    same = mc.same_bits(a, b)
    bad = np.flatnonzero(~same.all(1))
    print(f"{name}: {len(a)} inputs, {len(bad)} differ; {int((a[:, 6] == mc.SENTINEL).sum())} early-outs, {int(np.isnan(a).any(1).sum())} with a NaN")
    for i in bad[:5]:
        print(f"  input {i} (lane {i % mc.WAVE}) type {types[i]} wo {wo[i].tolist()} uu {uu[i].tolist()}\n    old {a[i].tolist()}\n    new {b[i].tolist()}")
    return bad


LAYOUT_NAMES = [f"type:{n}" for n in mc.TYPES] + [f"{k}:{p}" for k in ("seeded", "edge") for p in mc.PATTERNS] + ["edge_among_seeded"]


@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_stream_equals_separate_branches(mgpu, layouts, name):
    types, color, wo, uu = layouts[name]
    old = _s_f(mgpu, name, layouts[name], 0, mc.SENTINEL)
    new = _s_f(mgpu, name, layouts[name], 1, mc.SENTINEL)
    bad = _report(name, types, wo, uu, old, new)
    assert len(bad) == 0
    # the sentinel stays exactly where S_F returns early; nobody else returns it
    if name.startswith("type:") and name[5:] in ("emitter", "nil"):
        assert (old[:, 6] == mc.SENTINEL).all() and (old[:, :6] == 0).all()
    if name == "type:lambert":
        assert not (old[:, 6] == mc.SENTINEL).any()
    if name in ("type:metal", "type:plastic", "type:glass"):
        early = old[:, 6] == mc.SENTINEL
        assert 50 < early.sum() < len(old) // 2 and (old[early, 3:6] == 0).all()


def test_one_lane_gets_the_same_answer_in_every_company(mgpu, layouts):
    """a lane's result must not depend on who shares its wavefront: the Metal inputs of `seeded:metal_only` are the first ones of
    `type:metal`'s seeded set, and the interleaved layouts draw the same inputs again in other company"""
    ne = mc.inputs("metal")[2]
    alone = _s_f(mgpu, "type:metal", layouts["type:metal"], 1, mc.SENTINEL)[ne:]
    for name in ("seeded:metal_only", "seeded:both_halves", "seeded:interleaved", "seeded:both_one_metal_lane"):
        t = layouts[name][0]
        got = _s_f(mgpu, name, layouts[name], 1, mc.SENTINEL)[t == abi.MAT_METAL]
        assert mc.same_bits(got, alone[:len(got)]).all(), name


@pytest.mark.parametrize("stream", [0, 1], ids=["separate", "stream"])
@pytest.mark.parametrize("name", list(mc.TYPES))
def test_both_forms_match_the_oracle(mgpu, name, stream):
    """attenuation and pdf everywhere (the oracle's pdf starts as 0, so does the hook's here); wi wherever S_F got past its early-outs,
    and for Metal and the cosine lobe everywhere: on an early-out after the reflection the reference has already assigned wi, which
    beckmann_finish (Plastic, Glass) leaves for after it -- the integrators read wi of a sample with pdf 0 nowhere"""
    wo, uu = mc.oracle_inputs(name)
    n = len(wo)
    inputs = (np.full(n, mc.TYPES[name], np.uint32), np.tile(np.array(mc.COLOR, np.float32), (n, 1)), np.ascontiguousarray(wo), np.ascontiguousarray(uu))
    got = _s_f(mgpu, f"oracle:{name}", inputs, stream, 0.0)
    live = _s_f(mgpu, f"oracle:{name}", inputs, stream, mc.SENTINEL)[:, 6] != mc.SENTINEL
    ref = mc.oracle_s_f(name)
    same = mc.same_bits(got, ref)
    if name in ("plastic", "glass"):
        same[~live, :3] = True
    bad = np.flatnonzero(~same.all(1))
    print(f"{name} stream={stream}: {n} inputs, {int(live.sum())} past the early-outs, {len(bad)} differ from the oracle")
    for i in bad[:5]:
        print(f"  input {i} wo {wo[i].tolist()} uu {uu[i].tolist()}\n    gpu    {got[i].tolist()}\n    oracle {ref[i].tolist()}")
    assert len(bad) == 0


# ------------------------------------------------------------------------------------------------------------------ frames
def _frame(t, shape):
    """the config-2 scene through one shape of kernel -> (accum, rng, stats, kernel choice, oracle accum, oracle rng, oracle stats, mask)"""
    key = ("frame", shape)
    if key in _OUT:
        return _OUT[key]
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    scene = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    w, h, spp, nranks = (DENSE_W, DENSE_H, DENSE_SPP, DENSE_NRANKS) if shape == "dense" else (W, H, 2 if shape == "strip" else 16, 1)
    cam = host.prepare_camera(w, h)
    try:
        t.upload_scene(scene.view); t.upload_triangle_materials(None); t.upload_textures([])
        t.set_camera(cam); t.set_environment((0.0, 0.0, 0.0)); t.set_environment_map(None); t.resize(w, h)
        t.debug_set("strip_force", 2 if shape == "strip" else 0)
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        t.render(spp=spp, max_depth=8, integrator=abi.INTEGRATOR_PATH)
        got = t.download_accum(), t.download_rng(), t.stats(), t.last_kernel()
        t.debug_set("strip_force", 0); t.resize(W, H)
    except TracerError:
        FAULTED.append(f"frame-{shape}")
        raise
    ref_rng = host.fill_rng(SEED, w, h)
    ref, ref_st = po.render(scene.view, cam, w, h, ref_rng, spp=spp, max_depth=8, integrator=abi.INTEGRATOR_PATH, tile_rank=0, tile_nranks=nranks)
    ty, tx = np.mgrid[0:h, 0:w] // abi.TRC_TILE
    mask = ((tx + ty) % nranks) == 0
    _OUT[key] = got + (ref, ref_rng, ref_st, mask)
    return _OUT[key]


@pytest.mark.parametrize("shape", ["one", "strip", "dense"])
def test_frames_match_the_oracle(mgpu, shape):
    acc, rng, st, k, ref, ref_rng, ref_st, mask = _frame(mgpu, shape)
    bad = (acc.view(np.uint32) != ref.view(np.uint32)).any(-1) & mask
    print(f"{shape}: kernel {k}; {int(mask.sum())} pixels compared, {int(bad.sum())} differ; rays {st.rays} paths {st.paths} shaded {st.shaded}")
    assert k["shape"] == shape and k["variant"] == "plain" and k["lds_resident"] and not k["triangle_materials"], k
    assert k["strip"] == (2 if shape == "strip" else 1)
    assert np.isfinite(acc).all() and not bad.any()
    assert np.array_equal(rng[mask], ref_rng[mask])
    if shape == "dense":                    # the oracle rendered one tile in 64: its counters are that share's
        assert mask.sum() > 5000 and st.paths == DENSE_W * DENSE_H * DENSE_SPP and ref_st.paths == mask.sum() * DENSE_SPP
    else:
        assert (st.rays, st.paths, st.shaded) == (ref_st.rays, ref_st.paths, ref_st.shaded)
