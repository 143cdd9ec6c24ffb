"""The CPU side of TRC_FLAG_MATERIAL_PARAMS (include/tracer_abi.h): the scalar restatement of Material::S_F / Material::F with the lobe
parameters handed in (tests/material_params_ref/) is held to what exists -- at the default parameters to the oracle's Material_S_F /
Material_F, at any roughness to orc_microfacet (and to the reference's own headers compiled on the host, where oracle/_ref is built), at
any index to orc_fr_dielectric_n / orc_fr_conductor_n -- bit for bit; and trc_host_default_material_params to the literals parsed out of
the reference's sources.  The GPU tests (tests/test_gpu_material_params.py) then hold the kernels' parametrised lobes to the restatement."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import microfacet_cases as mc
from oracle import pyoracle as po
from tracer_amd import abi, host
from tracer_amd.dtypes import MATERIAL_PARAMS_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "material_params_ref"))
import material_params_loader as mpl  # noqa: E402

F = np.float32
N_RANDOM = 100000
# roughness pairs: the literals, random ones, the clamp's two sides (orc_microfacet's constructors clamp to 0.001 like the reference's)
ALPHAS = [(0.01, 0.1), (0.01, 0.01), (0.01, 0.02), (0.3, 0.3), (1.0, 0.001), (0.0005, 0.2), (0.0010001, 0.00099), (0.731, 0.0437), (0.05, 1.0)]


@pytest.fixture(scope="module")
def ref():
    return mpl.build()


@pytest.fixture(scope="module")
def pin():
    return po.Pin()


def _material(mtype):
    m = abi.Material()
    m.type = mtype
    m.textureInfo.type = abi.TEX_CONSTANT
    m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z = mc.COLOR
    return m


def _inputs(name):
    """(wo, wi, uu): the edge inputs of tests/microfacet_cases.py, then N_RANDOM seeded ones; wi: the edge directions in another order, then
    random directions, half of them near the mirror direction of wo (where the reflection lobes are not negligible)"""
    we, ue = mc.edge_inputs()
    ws, us = mc.seeded_inputs(2000 + list(mc.TYPES).index(name), N_RANDOM)
    wo, uu = np.concatenate([we, ws]), np.concatenate([ue, us])
    rs = np.random.RandomState(77 + list(mc.TYPES).index(name))
    wi = rs.normal(size=(len(wo), 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    mirror = wo.astype(np.float64) * np.array([-1.0, -1.0, 1.0]) + rs.normal(size=(len(wo), 3)) * (10.0 ** rs.uniform(-4, -1, (len(wo), 1)))
    mirror /= np.maximum(np.linalg.norm(mirror, axis=1, keepdims=True), 1e-30)
    wi = np.where((np.arange(len(wo)) % 2 == 0)[:, None], mirror, wi).astype(F)
    wi[:len(we)] = np.roll(we, 7, axis=0) * np.array([-1, 1, 1], F)
    return np.ascontiguousarray(wo), np.ascontiguousarray(wi), np.ascontiguousarray(uu)


def _all_same(got, want, what):
    same = mpl.same_bits(got, want)
    bad = np.argwhere(~same.all(axis=-1) if same.ndim > 1 else ~same)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} differ, first {bad[0]}: {got[bad[0][0]]} / {want[bad[0][0]]}"


@pytest.mark.parametrize("name", list(mc.TYPES))
def test_default_parameters_are_the_oracles_materials(ref, pin, name):
    mtype = mc.TYPES[name]
    wo, wi, uu = _inputs(name)
    n = len(wo)
    types, color = np.full(n, mtype, np.uint32), np.tile(np.array(mc.COLOR, F), (n, 1))
    params = np.repeat(host.default_material_params([mtype]), n)
    uv = np.zeros((n, 2), F)
    m = _material(mtype)
    got = ref.s_f(types, color, params, wo, uu)
    want = pin.material("s_f", m, wo, uv, uu)
    if name in ("plastic", "metal", "glass"):
        assert (want[:, 6] > 0).sum() > n // 4                                                  # the lobes are reached
    _all_same(got, want, f"S_F {name}")
    _all_same(ref.f(types, color, params, wo, wi, uu), pin.material("f", m, wo, wi, uv, uu), f"F {name}")


def _directions(seed, n):
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(n, 3))
    v[:, 2] *= np.where(np.arange(n) % 4 == 0, 10.0 ** rs.uniform(-5, -1, n), 1.0)
    v[:, :2] *= np.where(np.arange(n) % 4 == 1, 10.0 ** rs.uniform(-4, -1, n), 1.0)[:, None]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F)


@pytest.mark.parametrize("dist", (0, 1), ids=("beckmann", "trowbridge_reitz"))
def test_distributions_at_any_roughness(ref, pin, dist):
    we, ue = mc.edge_inputs()
    wo = np.concatenate([we, _directions(5, 20000)])
    uu = np.concatenate([ue, np.random.RandomState(6).uniform(0, 1, (20000, 2)).astype(F)])
    wh = np.concatenate([np.roll(we, 3, axis=0), _directions(7, 20000)])
    wh[:, 2] = np.abs(wh[:, 2])
    rs = np.random.RandomState(8)
    pairs = ALPHAS + [tuple(10.0 ** rs.uniform(-3, 0, 2)) for _ in range(6)]
    metal_ref = po.Pin(ref=True) if os.path.exists(po.METAL_REF) else None
    for ax, ay in pairs:
        ax, ay = float(F(ax)), float(F(ay))
        got = ref.microfacet(dist, ax, ay, wo, wh, uu)
        _all_same(got, pin.microfacet(dist, ax, ay, wo, wh, uu), f"orc_microfacet dist {dist} alpha ({ax}, {ay})")
        if metal_ref is not None:
            want = metal_ref.microfacet(dist, ax, ay, wo, wh, uu)
            want[:, 7] = got[:, 7] if dist == 0 else want[:, 7]         # Beckmann::Lambda is private in the reference: not compared
            _all_same(got, want, f"ref_microfacet dist {dist} alpha ({ax}, {ay})")


def test_fresnel_terms_at_any_index(ref, pin):
    rs = np.random.RandomState(9)
    n = 200000
    cosi = np.concatenate([np.array([0, -0.0, 1, -1, 1e-30, -1e-30, 1.5, -1.5, 0.5, 1e-4], F), rs.uniform(-1.01, 1.01, n).astype(F)])
    n = len(cosi)
    eta = np.concatenate([np.array([1.5, 1.3, 1.05, 2.5, 1.0000001], F), rs.uniform(1.0, 2.6, n - 5).astype(F)])
    _all_same(ref.fr_dielectric(cosi, eta), pin.map("fr_dielectric_n", 1, cosi, eta)[:, 0], "FrDielectric")
    e3, k3 = rs.uniform(0.1, 4.0, (n, 3)).astype(F), rs.uniform(0.1, 4.0, (n, 3)).astype(F)
    e3[:4], k3[:4] = (0.18, 0.15, 0.81), (1.0, 1.0, 1.0)
    _all_same(ref.fr_conductor(np.abs(cosi), e3, k3), pin.map("fr_conductor_n", 3, np.abs(cosi), e3, k3), "FrConductor")


def test_parameters_change_the_lobes(ref):
    """the restatement reads what it is handed: another roughness, index or conductor changes the lobe that uses it and no other"""
    wo, _, uu = _inputs("metal")
    wo, uu = wo[-4096:], uu[-4096:]
    n = len(wo)
    color = np.tile(np.array(mc.COLOR, F), (n, 1))
    for name, field, value, touched in (("metal", "alpha_y", 0.3, True), ("metal", "eta", 1.3, False), ("metal", "metal_k", (2.0, 2.0, 2.0), True),
                                        ("glass", "eta", 1.3, True), ("glass", "metal_eta", (1.0, 1.0, 1.0), False),
                                        ("plastic", "alpha_x", 0.2, True), ("lambert", "alpha_x", 0.2, False), ("lambert", "eta", 2.0, False)):
        types = np.full(n, mc.TYPES[name], np.uint32)
        p0 = np.repeat(host.default_material_params([mc.TYPES[name]]), n)
        p1 = p0.copy()
        p1[field] = value
        differ = not mpl.same_bits(ref.s_f(types, color, p0, wo, uu), ref.s_f(types, color, p1, wo, uu)).all()
        assert differ == touched, (name, field)


def test_host_defaults_are_the_references_literals():
    consts = json.load(open(os.path.join(_HERE, "golden", "reference_constants.json")))["functions"]
    d = host.default_material_params([abi.MAT_PLASTIC, abi.MAT_GLASS, abi.MAT_METAL, abi.MAT_LAMBERT, abi.MAT_DIFFUSE, abi.MAT_NIL, 77])
    ax, ay, eta, _ = consts["createPlasticMaterial"]                     # Beckmann(ax, ay), FresnelDielectric(eta), R
    assert (d[0]["alpha_x"], d[0]["alpha_y"], d[0]["eta"]) == (F(ax), F(ay), F(eta))
    eta, ax, ay = consts["createGlass"]
    assert (d[1]["alpha_x"], d[1]["alpha_y"], d[1]["eta"]) == (F(ax), F(ay), F(eta))
    ax, ay, e0, e1, e2, k = consts["createMetalMaterial"]
    assert (d[2]["alpha_x"], d[2]["alpha_y"]) == (F(ax), F(ay))
    assert tuple(d[2]["metal_eta"]) == (F(e0), F(e1), F(e2)) and tuple(d[2]["metal_k"]) == (F(k), F(k), F(k))
    for other in d[3:]:                                                  # any other type: Plastic's values
        assert other.tobytes() == d[0].tobytes()
    for rec in d:                                                        # every record of defaults is a valid one
        assert rec["alpha_x"] > 0 and rec["alpha_y"] > 0 and rec["eta"] > 1 and (rec["metal_eta"] > 0).all() and (rec["metal_k"] > 0).all()
        assert rec["_pad0"] == 0 and rec["_pad1"] == 0 and rec["_pad2"] == 0


def test_mirror_of_the_header():
    text = open(os.path.join(os.path.dirname(_HERE), "include", "tracer_abi.h")).read()
    assert int(re.search(r"#define TRC_FLAG_MATERIAL_PARAMS\s+(\d+)u", text).group(1)) == abi.FLAG_MATERIAL_PARAMS == 256
    assert C.sizeof(abi.MaterialParams) == 48 == MATERIAL_PARAMS_DTYPE.itemsize
    assert abi.MaterialParams.metal_eta.offset == 16 == MATERIAL_PARAMS_DTYPE.fields["metal_eta"][1]
    assert abi.MaterialParams.metal_k.offset == 32 == MATERIAL_PARAMS_DTYPE.fields["metal_k"][1]
    flags = [int(v) for v in re.findall(r"#define TRC_FLAG_\w+\s+(\d+)u", text)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)      # one bit each, none shared
