"""The input generator of the microfacet-stream tests (tests/microfacet_cases.py) held to its own conditions, without a GPU: every
mixture of lobe families in a wavefront is present, every edge value the tests promise is present, and the oracle says that neither
side of a lobe's early-outs goes untested."""
import numpy as np
import pytest

import microfacet_cases as mc
from tracer_amd import abi

F32 = np.float32


@pytest.fixture(scope="module")
def layouts():
    return mc.layouts(mix_waves=64)


def _families(types):
    """per wavefront: (has Metal lanes, has Beckmann lanes, number of distinct materials)"""
    t = types.reshape(-1, mc.WAVE)
    metal = (t == abi.MAT_METAL).any(1)
    beck = ((t == abi.MAT_PLASTIC) | (t == abi.MAT_GLASS)).any(1)
    return metal, beck, np.array([len(set(r)) for r in t])


def test_every_mixture_pattern_is_present(layouts):
    for kind in ("seeded", "edge"):
        m, b, _ = _families(layouts[f"{kind}:metal_only"][0]); assert m.all() and not b.any()
        m, b, _ = _families(layouts[f"{kind}:beckmann_only"][0]); assert b.all() and not m.any()
        for name in ("both_halves", "both_one_metal_lane", "both_one_beckmann_lane"):
            m, b, _ = _families(layouts[f"{kind}:{name}"][0]); assert (m & b).all()
        t = layouts[f"{kind}:interleaved"][0].reshape(-1, mc.WAVE)
        assert (t[:, :4] == [abi.MAT_LAMBERT, abi.MAT_PLASTIC, abi.MAT_METAL, abi.MAT_GLASS]).all() and (t[:, 4:8] == t[:, :4]).all()
        m, b, k = _families(layouts[f"{kind}:interleaved_all"][0]); assert (m & b).all() and (k == 6).all()
    t = layouts["seeded:both_one_metal_lane"][0].reshape(-1, mc.WAVE); assert ((t == abi.MAT_METAL).sum(1) == 1).all()
    t = layouts["seeded:both_one_beckmann_lane"][0].reshape(-1, mc.WAVE); assert ((t != abi.MAT_METAL).sum(1) == 1).all()
    for name, mt in mc.TYPES.items():
        t, c, wo, uu = layouts[f"type:{name}"]
        assert (t == mt).all() and len(t) == mc.inputs(name)[2] + mc.N_SEEDED and len(t) % mc.WAVE == 0
    for t, c, wo, uu in layouts.values():
        assert len(t) % mc.WAVE == 0 and c.shape == (len(t), 3) and wo.shape == (len(t), 3) and uu.shape == (len(t), 2)
        assert t.dtype == np.uint32 and wo.dtype == F32 and uu.dtype == F32


def test_edge_lane_among_seeded_lanes(layouts):
    t, c, wo, uu = layouts["edge_among_seeded"]
    n_edge = mc.inputs("metal")[2]
    assert len(t) == n_edge * mc.WAVE
    names = mc.PATTERNS["interleaved"]
    lanes = set()
    for w in (0, 1, 17, n_edge - 1):
        lane = (w * 7) % mc.WAVE
        ew, eu, _ = mc.inputs(names[lane])
        assert np.array_equal(wo[w * mc.WAVE + lane].view(np.uint32), ew[w].view(np.uint32)) and np.array_equal(uu[w * mc.WAVE + lane], eu[w])
        lanes.add(lane)
    assert len({(w * 7) % mc.WAVE for w in range(mc.WAVE)}) == mc.WAVE        # the edge lane visits every lane, so every material


def test_every_edge_value_is_present():
    d = mc.edge_wo()
    wo = np.array(list(d.values()), F32)
    z = wo[:, 2]
    bits = z.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any()                                     # +0 and -0
    den = (z != 0) & (np.abs(z) < np.finfo(F32).tiny)
    assert (z[den] > 0).any() and (z[den] < 0).any()                                            # denormal
    assert (z == 1).any() and (z == -1).any() and (z == mc.ONE_M).any() and (z == -mc.ONE_M).any()
    assert ((wo[:, 0] == 0) & (wo[:, 1] != 0)).any() and ((wo[:, 1] == 0) & (wo[:, 0] != 0)).any()
    n = np.linalg.norm(wo.astype(np.float64), axis=1)
    assert np.abs(n - 1)[~den & (z != 0)].max() < 1e-6
    # the stretched cosine lies on both sides of 0.9999 under every roughness pair a lobe stretches with, within 3e-7 (five ulps) of it
    for ay in mc.ALPHAS:
        c = mc.stretched_cos(wo, 0.01, ay)
        hi, lo = c[c > mc.COS_SPLIT], c[c <= mc.COS_SPLIT]
        assert len(hi) and len(lo) and hi.min() - mc.COS_SPLIT < 3e-7 and mc.COS_SPLIT - lo.max() < 3e-7, (ay, hi.min(), lo.max())
    uu = mc.edge_uu()
    for v in (0.0, 0.25, 0.5, 1.0, mc.ONE_M, mc.ulps(F32(0.25), -1), mc.ulps(F32(0.25), 1), mc.ulps(F32(0.5), -1), mc.ulps(F32(0.5), 1)):
        assert (uu[:, 0] == F32(v)).any(), v
    for v in (0.0, 1.0, mc.ONE_M):
        assert (uu[:, 1] == F32(v)).any(), v
    ew, eu = mc.edge_inputs()
    assert len(ew) == len(wo) * len(uu) and len(ew) % mc.WAVE == 0
    for name in mc.TYPES:                    # the edge set leads every type's inputs, and the seeded set is seeded
        w, u, ne = mc.inputs(name)
        assert ne == len(ew) and np.array_equal(w[:ne].view(np.uint32), ew.view(np.uint32)) and np.array_equal(u[:ne], eu)
    a, b = mc.seeded_inputs(5, 1000), mc.seeded_inputs(5, 1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] < 1).all()


@pytest.mark.parametrize("lobe", list(mc.LOBES))
def test_both_sides_of_the_early_outs(lobe):
    """an early-out of S_F leaves pdf and attenuation 0 in the oracle (whose pdf starts as 0); between 5 % and 60 % of the inputs a
    lobe gets must end so, with some in the edge set and some in the seeded set -- and some must sample a wh with dot(wo, wh) <= 0"""
    name, lo, hi = mc.LOBES[lobe]
    wo, uu = mc.oracle_inputs(name)
    ne = mc.inputs(name)[2]
    out = mc.oracle_s_f(name)
    mine = (uu[:, 0] >= lo) & (uu[:, 0] < hi)
    early = (out[:, 6] == 0) & (out[:, 3:6] == 0).all(1)
    for part, sel in (("edge", np.arange(len(wo)) < ne), ("seeded", np.arange(len(wo)) >= ne), ("all", np.arange(len(wo)) >= 0)):
        frac = early[mine & sel].mean()
        print(f"{lobe} {part}: {int((mine & sel).sum())} inputs, {100 * frac:.1f} % early-outs")
        assert early[mine & sel].sum() >= 50          # each part holds early-outs of its own
    assert 0.05 <= frac <= 0.60, (lobe, frac)
    if lobe in ("metal", "plastic_specular"):
        # wi stays 0 where the first early-out (dot(wo, wh) <= 0) was taken.  Glass's isotropic (0.01, 0.01) samples no such wh from
        # these inputs; its reflection lobe runs the same instructions as Plastic's.
        first = early & mine & (out[:, :3] == 0).all(1) & (wo[:, 2] != 0)
        print(f"{lobe}: {int(first.sum())} inputs leave wi untouched")
        assert first.sum() >= 50
