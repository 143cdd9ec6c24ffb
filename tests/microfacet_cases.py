"""Inputs of material_S_F for tests/test_gpu_microfacet_stream.py (the device hook trc_material_s_f_test, both forms of the lobe code)
and tests/test_microfacet_cases.py (which holds this generator to its own conditions on the CPU, with the oracle).

An input is (material type, colour, wo in the shading frame, the two random numbers).  Per material type there are a seeded set and
an edge set; layouts() arranges them by wavefront (64 consecutive inputs run as one wavefront of the hook's kernel), so that the
wave-uniform guards of the merged stream (the __ballot fall-backs of rcp_cr, sqrt_cr, div_const2) see one family alone, every mixture
of families, and one out-of-range lane among ordinary ones."""
from collections import OrderedDict

import numpy as np

from tracer_amd import abi

F32 = np.float32
WAVE = 64
N_SEEDED = 1 << 18
N_ORACLE = 4096                      # seeded inputs per type that are also held to the oracle
SENTINEL = F32(-7.0)                 # pdf_out before the call: no lobe returns a negative pdf
COLOR = (0.73, 0.4, 0.2)
TYPES = OrderedDict([("lambert", abi.MAT_LAMBERT), ("plastic", abi.MAT_PLASTIC), ("metal", abi.MAT_METAL), ("glass", abi.MAT_GLASS),
                     ("emitter", abi.MAT_DIFFUSE), ("nil", abi.MAT_NIL)])
# the lobes with early-outs and who runs them: Plastic's specular half (uu.x >= 0.5), Metal, Glass reflection (uu.x < 0.25) / transmission
LOBES = OrderedDict([("metal", ("metal", 0.0, 2.0)), ("plastic_specular", ("plastic", 0.5, 2.0)),
                     ("glass_reflection", ("glass", 0.0, 0.25)), ("glass_transmission", ("glass", 0.25, 2.0))])
COS_SPLIT = F32(0.9999)              # sample11's corner: the cosine of the STRETCHED direction
ALPHAS = (0.01, 0.02, 0.1)           # every roughness a lobe stretches with (x is 0.01 for all, y one of the three)
DENORMAL = F32(1e-40)


def ulps(x, k):
    return (np.array(x, F32).view(np.int32) + np.int32(k)).view(F32)[()]


ONE_M = ulps(F32(1.0), -1)           # 1 - ulp
U_X = [F32(0), F32(1e-7), ulps(F32(0.25), -1), F32(0.25), ulps(F32(0.25), 1), ulps(F32(0.5), -1), F32(0.5), ulps(F32(0.5), 1),
       ONE_M, F32(1.0), F32(0.1), F32(0.3), F32(0.7), F32(0.9),
       F32(1e-12), F32(0.2499997), F32(0.2500003), F32(0.5000006), F32(0.999999)]       # the tails of the lobes' intervals
U_Y = [F32(0), ulps(F32(0.5), -1), F32(0.5), ulps(F32(0.5), 1), ONE_M, F32(1.0), F32(0.3), F32(0.8)]


def edge_uu():
    return np.array([(x, y) for x in U_X for y in U_Y], F32)


def _unit(x, y, z):
    v = np.array([x, y, z], np.float64)
    return tuple((v / np.linalg.norm(v)).astype(F32))


def edge_wo():
    """name -> direction; the names say which condition of the issue a direction is there for"""
    d = OrderedDict()
    for s, sign in (("+", 1.0), ("-", -1.0)):
        d[f"z{s}0"] = (F32(0.6), F32(0.8), F32(sign * 0.0))
        d[f"z{s}denormal"] = (F32(0.6), F32(0.8), F32(sign) * DENORMAL)
        d[f"z{s}1"] = (F32(0), F32(0), F32(sign))
        r = np.sqrt(1.0 - float(ONE_M) ** 2)
        d[f"z{s}1-ulp"] = (F32(r * 0.6), F32(r * 0.8), F32(sign) * ONE_M)
        for th in (0.3, 1.0, 1.5):
            d[f"x0{s}{th}"] = (F32(0), F32(np.sin(th)), F32(sign * np.cos(th)))
            d[f"y0{s}{th}"] = (F32(np.sin(th)), F32(0), F32(sign * np.cos(th)))
        # the stretched cosine on both sides of 0.9999: a direction in the xz- or yz-plane whose tangent, times alpha, is the split's
        t_split = np.sqrt(1.0 / float(COS_SPLIT) ** 2 - 1.0)
        for a in ALPHAS:
            for axis in ("x", "y") if a == 0.01 else ("y",):
                for k, delta in enumerate((-1e-2, -2e-3, -6e-4, 6e-4, 2e-3, 1e-2)):
                    t = t_split / a * (1.0 + delta)
                    v = _unit(t, 0, sign) if axis == "x" else _unit(0, t, sign)
                    d[f"split{s}{axis}{a}:{k}"] = v
        # grazing: the sampled wh easily has dot(wo, wh) <= 0
        for z in (1e-30, 1e-20, 1e-10, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2):
            d[f"graze{s}{z}"] = _unit(0.8, -0.6, sign * z)
    return d


def stretched_cos(wo, ax, ay):
    """cos_theta of sample_wh's wiStretched, evaluated as the kernels do (float32, left to right)"""
    wo = np.asarray(wo, F32)
    w = np.where(wo[:, 2:3] < 0, -wo, wo)
    x, y, z = F32(ax) * w[:, 0], F32(ay) * w[:, 1], w[:, 2]
    inv = F32(1) / np.sqrt(x * x + y * y + z * z, dtype=F32)
    return z * inv


def edge_inputs():
    """(wo, uu): every edge direction with every edge pair of random numbers"""
    wo = np.array(list(edge_wo().values()), F32)
    uu = edge_uu()
    return np.repeat(wo, len(uu), 0), np.tile(uu, (len(wo), 1))


def seeded_inputs(seed, n=N_SEEDED):
    """(wo, uu): uniform directions, three in eight pressed towards the horizon and an eighth towards the normal; uu uniform in [0, 1),
    but for a quarter of the inputs (grazing ones) uu.x lies within 1e-3 ... 1e-9 of an end of its lobe's interval: visible-normal
    sampling gives next to no early-out elsewhere (0.1 % for Metal even at wo.z = 1e-5); the slopes of those tails do"""
    rs = np.random.RandomState(seed)
    wo = rs.normal(size=(n, 3))
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    k = np.arange(n) % 8
    wo[:, 2] *= np.where(k <= 2, 10.0 ** rs.uniform(-5, -1, n), 1.0)
    wo[:, :2] *= np.where(k == 3, 10.0 ** rs.uniform(-4, -1, n), 1.0)[:, None]
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    uu = rs.uniform(0, 1, (n, 2))
    tail = 10.0 ** rs.uniform(-9, -3, n)
    for lo, hi in ((0.0, 0.25), (0.25, 0.5), (0.5, 1.0)):       # the ends of every interval that material_S_F rescales to [0, 1)
        sel = (k < 2) & (uu[:, 0] >= lo) & (uu[:, 0] < hi)
        up = rs.uniform(0, 1, n) < 0.5
        uu[:, 0] = np.where(sel, np.where(up, hi - (hi - lo) * tail, lo + (hi - lo) * tail), uu[:, 0])
    uu = uu.astype(F32)
    uu[uu >= 1] = ONE_M
    return wo.astype(F32), uu


_CACHE = {}


def inputs(name):
    """(wo, uu, n_edge) of one material type: the edge set first, then the seeded set"""
    if name not in _CACHE:
        we, ue = edge_inputs()
        ws, us = seeded_inputs(1000 + list(TYPES).index(name))
        _CACHE[name] = (np.concatenate([we, ws]), np.concatenate([ue, us]), len(we))
    return _CACHE[name]


def _pack(parts):
    """parts: list of (type name, wo, uu) -> (types, color, wo, uu)"""
    t = np.concatenate([np.full(len(w), TYPES[n], np.uint32) for n, w, _ in parts])
    wo, uu = np.concatenate([w for _, w, _ in parts]), np.concatenate([u for _, _, u in parts])
    return t, np.tile(np.array(COLOR, F32), (len(t), 1)), np.ascontiguousarray(wo), np.ascontiguousarray(uu)


def _lanes(pattern, waves, take):
    """one wavefront after the other with lane l running type pattern[l]; take[name] hands out that type's inputs in order"""
    assert len(pattern) == WAVE
    names = sorted(set(pattern))
    count = {n: pattern.count(n) for n in names}
    lane = {n: np.array([l for l, p in enumerate(pattern) if p == n]) for n in names}
    types = np.zeros(waves * WAVE, np.uint32)
    wo, uu = np.zeros((waves * WAVE, 3), F32), np.zeros((waves * WAVE, 2), F32)
    for n in names:
        w, u = take(n, waves * count[n])
        idx = (np.arange(waves)[:, None] * WAVE + lane[n][None, :]).reshape(-1)
        types[idx], wo[idx], uu[idx] = TYPES[n], w, u
    return types, np.tile(np.array(COLOR, F32), (len(types), 1)), wo, uu


PATTERNS = OrderedDict([
    ("metal_only", ["metal"] * 64),
    ("beckmann_only", ["plastic", "glass"] * 32),
    ("both_halves", ["metal"] * 32 + ["plastic"] * 16 + ["glass"] * 16),
    ("both_one_metal_lane", ["plastic"] * 31 + ["metal"] + ["glass"] * 32),
    ("both_one_beckmann_lane", ["metal"] * 40 + ["glass"] + ["metal"] * 23),
    ("interleaved", ["lambert", "plastic", "metal", "glass"] * 16),
    ("interleaved_all", ["lambert", "plastic", "metal", "glass", "emitter", "nil", "metal", "glass"] * 8),
])


def layouts(mix_waves=1024):
    """name -> (types, color, wo, uu).  `type:<name>`: one type alone, its edge set and its 2^18 seeded inputs.  The PATTERNS, twice:
    on seeded inputs, and on the edge sets (an edge lane beside edge lanes of the other families).  `edge_among_seeded`: the four
    materials interleaved on seeded inputs with ONE edge input per wavefront, its lane moving from wavefront to wavefront."""
    out = OrderedDict()
    for n in TYPES:
        wo, uu, _ = inputs(n)
        out[f"type:{n}"] = _pack([(n, wo, uu)])

    def seeded(n, k):
        wo, uu, ne = inputs(n)
        assert ne + k <= len(wo)
        return wo[ne:ne + k], uu[ne:ne + k]

    def edges(n, k):
        wo, uu, ne = inputs(n)
        idx = np.arange(k) % ne
        return wo[idx], uu[idx]

    n_edge = inputs("metal")[2]
    for name, pat in PATTERNS.items():
        out[f"seeded:{name}"] = _lanes(pat, mix_waves, seeded)
        out[f"edge:{name}"] = _lanes(pat, -(-n_edge // min(pat.count(n) for n in set(pat))), edges)      # every type sees its whole edge set
    t, c, wo, uu = _lanes(PATTERNS["interleaved"], n_edge, seeded)
    t, wo, uu = t.copy(), wo.copy(), uu.copy()
    names = PATTERNS["interleaved"]
    for w in range(n_edge):
        lane = (w * 7) % WAVE
        ew, eu, _ = inputs(names[lane])
        wo[w * WAVE + lane], uu[w * WAVE + lane] = ew[w], eu[w]
    out["edge_among_seeded"] = (t, c, wo, uu)
    return out


def oracle_material(mtype):
    m = abi.Material()
    m.type, m.eta, m.roughness = mtype, 1.5, 0.5
    m.textureInfo.type = abi.TEX_CONSTANT
    m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z = COLOR
    return m


def oracle_inputs(name):
    """(wo, uu) held to the oracle: the edge set and the first N_ORACLE seeded inputs"""
    wo, uu, ne = inputs(name)
    return wo[:ne + N_ORACLE], uu[:ne + N_ORACLE]


_ORACLE = {}


def oracle_s_f(name):
    """(n, 7): wi, attenuation, pdf of the oracle's Material::S_F (wi and pdf start as 0) on oracle_inputs(name); computed once"""
    if name not in _ORACLE:
        from oracle import pyoracle as po
        wo, uu = oracle_inputs(name)
        _ORACLE[name] = po.Pin().material("s_f", oracle_material(TYPES[name]), wo, np.zeros((len(wo), 2), F32), uu)
        _ORACLE[name].setflags(write=False)
    return _ORACLE[name]


def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN (a NaN's sign and payload are whatever the last operation's operand order made
    them: tests/test_gpu_unary.py and the hooks count NaN == NaN the same way)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
