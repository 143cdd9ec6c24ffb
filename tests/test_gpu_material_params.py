"""TRC_FLAG_MATERIAL_PARAMS (include/tracer_abi.h): the lobe parameters the reference writes as literals are read per material from the
context's table.  The oracle renders the literals only, so nothing here needs an oracle frame of other parameters: the kernels'
parametrised lobes are held to the scalar restatement (tests/material_params_ref/, which tests/test_material_params_ref.py holds to the
oracle), and the flagged launch to the unflagged one, which is held to the oracle -- with a table of trc_host_default_material_params a
flagged render IS the unflagged one, bit for bit, on all 16 kernels (identity).  Then: which entry a lane reads (indexing), that the
parameters reach the picture, the flag under a tile mask / tile ranks / trc_render_adaptive, refusals and the table's lifetime.

Scenes of the kernel census (light_oracle_cases.cornell): Cornell + the 48-triangle ball (the tree in LDS) or the larger one (read from
memory), 61 x 45, 8 samples.  Everything is compared as uint32.  After a launch that left an error behind nothing more of this module runs
on the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import light_oracle_cases as lc
import microfacet_cases as mc
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError
from tracer_amd.dtypes import MATERIAL_PARAMS_DTYPE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "material_params_ref"))
import material_params_loader as mpl  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SEED, SPP = lc.W, lc.H, lc.SEED, 8
N = W * H
INTEGRATORS = {"path": lc.PATH, "mis": lc.MIS}
FAULTED = []
N_SEEDED = 1 << 13          # seeded inputs per material type of the lobe test, beside the edge set


@pytest.fixture(scope="module")
def rgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def u32(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)


def _types(view):
    return [view.materials[i].type for i in range(view.n_material)]


def _defaults(view):
    return host.default_material_params(_types(view))


def _upload(t, s, view=None, tri="scene"):
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    t.upload_scene(view if view is not None else s.view); t.upload_triangle_materials(s.tri if isinstance(tri, str) else tri); t.upload_textures(s.images)
    t.set_camera(s.cam); t.set_environment(lc.ENV_RGB); t.set_environment_map(None); t.resize(W, H)


def _frame(t, what, integrator, flagged, spp=SPP, calls=1, **kw):
    """seed the RNG texture, clear the accumulator, `calls` launches of spp / calls samples -> (accum, rng, stats)"""
    try:
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        for c in range(calls):
            t.render(spp=spp // calls, integrator=integrator, frame0=c * (spp // calls), material_params=flagged, **kw)
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


def _with_materials(s, extra=0):
    """a copy of a scene's view with a material array of its own (`extra` more entries, copies of entry 0): the cached scene stays as it is"""
    v = abi.Scene.from_buffer_copy(s.view)
    mats = (abi.Material * (v.n_material + extra))()
    for i in range(v.n_material + extra):
        mats[i] = s.view.materials[i if i < v.n_material else 0]
    v.materials = C.cast(mats, C.POINTER(abi.Material))
    v.n_material += extra
    v._keep = mats
    return v


def _refused(fn, status):
    with pytest.raises(TracerError) as e:
        fn()
    assert e.value.status == status, e.value


# ---------------------------------------------------------------------- 3. the lobes against the restatement
def _lobe_inputs():
    """64-lane groups: first every wavefront a mixture of Lambert, Plastic, Metal and Glass lanes, then wavefronts of one family alone; each
    type runs its edge set (tests/microfacet_cases.py) and N_SEEDED seeded inputs"""
    per = {}
    for name in ("lambert", "plastic", "metal", "glass"):
        we, ue = mc.edge_inputs()
        ws, us = mc.seeded_inputs(3000 + list(mc.TYPES).index(name), N_SEEDED)
        per[name] = (np.concatenate([we, ws]), np.concatenate([ue, us]))
    n = len(per["metal"][0])
    types = np.tile(np.array([mc.TYPES[k] for k in ("lambert", "plastic", "metal", "glass")], np.uint32), n)
    wo = np.stack([per[k][0] for k in ("lambert", "plastic", "metal", "glass")], 1).reshape(-1, 3)
    uu = np.stack([per[k][1] for k in ("lambert", "plastic", "metal", "glass")], 1).reshape(-1, 2)
    order = np.concatenate([np.arange(4 * n), np.argsort(types, kind="stable")])          # mixed, then sorted by family
    types, wo, uu = types[order], wo[order], uu[order]
    other = np.array([mc.TYPES["emitter"], mc.TYPES["nil"]] * 32, np.uint32)               # a wavefront of types without a lobe
    types = np.concatenate([types, other]); wo = np.concatenate([wo, wo[:64]]); uu = np.concatenate([uu, uu[:64]])
    rs = np.random.RandomState(12)
    wi = rs.normal(size=(len(wo), 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    mirror = wo.astype(np.float64) * np.array([-1.0, -1.0, 1.0]) + rs.normal(size=(len(wo), 3)) * (10.0 ** rs.uniform(-4, -0.5, (len(wo), 1)))
    through = -wo.astype(np.float64) + rs.normal(size=(len(wo), 3)) * (10.0 ** rs.uniform(-3, -0.5, (len(wo), 1)))      # near the refracted side
    pick = np.arange(len(wo)) % 3
    wi = np.where((pick == 0)[:, None], mirror, np.where((pick == 1)[:, None], through, wi))
    wi /= np.maximum(np.linalg.norm(wi, axis=1, keepdims=True), 1e-30)
    color = np.tile(np.array(mc.COLOR, F), (len(types), 1))
    return types, color, np.ascontiguousarray(wo, F), np.ascontiguousarray(wi.astype(F)), np.ascontiguousarray(uu, F)


def _report(got, want, what, types=None, wi_live=None):
    """rows of got and want with the same bits (a NaN equal to a NaN); prints the count, per material type, and the first rows that differ.
    wi_live: rows whose S_F got past its early-outs -- on an early-out after the reflection the reference has already assigned wi, which
    the kernels' microfacet_finish leaves for after it for the Beckmann lobes (Plastic, Glass): the integrators read wi of a sample with
    pdf 0 nowhere, and tests/test_gpu_microfacet_stream.py compares the existing lobes with the oracle under the same rule"""
    same = mpl.same_bits(got, want)
    if wi_live is not None:
        same[(~wi_live & ((types == abi.MAT_PLASTIC) | (types == abi.MAT_GLASS))), :3] = True
    same = same.all(axis=1)
    by_type = "" if types is None else ", by type " + str({int(k): int(((types == k) & ~same).sum()) for k in np.unique(types)})
    print(f"{what}: {int((~same).sum())} of {len(same)} inputs differ{by_type}")
    for i in np.flatnonzero(~same)[:4]:
        print(f"  input {i} type {None if types is None else types[i]}\n    gpu  {got[i].tolist()}\n    want {want[i].tolist()}")
    return same


def test_the_parametrised_lobes_equal_the_restatement(rgpu):
    t, ref = rgpu, mpl.build()
    if FAULTED:
        pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
    types, color, wo, wi, uu = _lobe_inputs()
    n = len(types)
    params = mpl.random_params(np.random.RandomState(13), n)
    params[::97] = host.default_material_params(types[::97])           # some lanes at the literals among the random ones
    ok = {}
    try:
        want = ref.s_f(types, color, params, wo, uu, pdf_init=mc.SENTINEL)
        live = want[:, 6] != mc.SENTINEL
        for mt in (abi.MAT_METAL, abi.MAT_GLASS, abi.MAT_PLASTIC):             # the lobes are reached, and so are their early-outs
            assert (want[:, 6] > 0)[types == mt].sum() > 8 * N_SEEDED // 10 and (~live)[types == mt].sum() > 50
        for op, name in ((0, "S_F"), (2, "S_F, sample11 once")):
            got = t.material_params_test(op, types, color, params, wo, uu, pdf_init=mc.SENTINEL)
            assert np.array_equal(got[:, 6] != mc.SENTINEL, live)                # the early-outs are the restatement's
            ok[name] = _report(got, want, f"op {op} ({name}), random parameters", types, live).all()
        got = t.material_params_test(1, types, color, params, wo, uu, wi=wi)
        want = ref.f(types, color, params, wo, wi, uu)
        for mt in (abi.MAT_METAL, abi.MAT_GLASS, abi.MAT_PLASTIC):             # F is reached with a non-trivial value
            assert ((want[:, 3] > 0) & (types == mt)).sum() > 1000
        ok["F"] = _report(got, want, "op 1 (F), random parameters", types).all()
        # at the default parameters: the existing lobe code (trc_material_s_f_test, the stream form), and the restatement again
        d = host.default_material_params(types)
        got = t.material_params_test(0, types, color, d, wo, uu, pdf_init=mc.SENTINEL)
        ok["defaults, material_S_F"] = _report(got, t.material_s_f_test(types, color, wo, uu, 1, pdf_init=mc.SENTINEL), "op 0 at the defaults against material_S_F", types).all()
        want = ref.s_f(types, color, d, wo, uu, pdf_init=mc.SENTINEL)
        ok["defaults, restatement"] = _report(got, want, "op 0 at the defaults against the restatement", types, want[:, 6] != mc.SENTINEL).all()
    except TracerError:
        FAULTED.append("lobes")
        raise
    assert all(ok.values()), ok


# ---------------------------------------------------------------------- 4. identity, all 16 kernels
@pytest.mark.parametrize("tex", (False, True), ids=("notex", "tex"))
@pytest.mark.parametrize("trimat", (False, True), ids=("plain19", "trimat"))
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_default_parameters_give_the_unflagged_render(rgpu, residence, trimat, tex):
    t, s = rgpu, lc.cornell(residence, tex, trimat)
    _upload(t, s)
    t.upload_material_params(_defaults(s.view))
    for name, integ in INTEGRATORS.items():
        for calls in (1, SPP):              # 8 samples in one call; 8 calls of 1 sample, coalesced
            what = f"{residence}-{'trimat' if trimat else 'plain19'}-{'tex' if tex else 'notex'}-{name}-{calls}x{SPP // calls}"
            want = _frame(t, what, integ, False, calls=calls)
            assert not t.last_material_params()
            got = _frame(t, what, integ, True, calls=calls)
            k = t.last_kernel()
            assert t.last_material_params() and not t.last_camera_rays(), k
            assert k["shape"] == "one" and k["variant"] == ("tex" if tex else "plain") and k["strip"] == 1, k
            assert k["lds_resident"] == (residence == "lds") and k["triangle_materials"] == trimat, k
            assert want[2][1] == N * SPP
            _same(got, want, what)


# ---------------------------------------------------------------------- 5. indexing
@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_a_lane_reads_its_own_materials_entry(rgpu, residence):
    """Cornell's 20 entries are all named by some primitive but entry 1 (spheres 7 .. 18, squares 3 .. 6, cubes 0, 19, 2), so the two
    Plastic records that only triangles name are entries 20 and 21 of a table two entries longer."""
    t, s = rgpu, lc.cornell(residence, False, True)
    v = _with_materials(s, extra=2)
    a, b = v.n_material - 2, v.n_material - 1
    for prims, count in ((v.sphereList, v.n_sphere), (v.squareList, v.n_square), (v.cubeList, v.n_cube)):
        assert all(prims[i].material < a for i in range(count))
    for slot, albedo in ((a, (0.7, 0.6, 0.3)), (b, (0.3, 0.5, 0.8))):
        m = v.materials[slot]
        m.type = abi.MAT_PLASTIC
        m.textureInfo.type = abi.TEX_CONSTANT
        m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z = albedo
    tri = s.tri.copy()
    tri[0::3], tri[1::3] = a, b
    table = _defaults(v)
    table[a]["alpha_x"], table[a]["alpha_y"], table[a]["eta"] = 0.2, 0.05, 1.3
    table[b]["alpha_x"], table[b]["alpha_y"], table[b]["eta"] = 0.02, 0.4, 2.0
    _upload(t, s, view=v, tri=tri)
    t.upload_material_params(table)
    first = {name: _frame(t, f"index-{residence}-{name}", integ, True) for name, integ in INTEGRATORS.items()}
    # the table's two entries alone swapped: another picture
    swapped = table.copy()
    swapped[[a, b]] = table[[b, a]]
    t.upload_material_params(swapped)
    for name, integ in INTEGRATORS.items():
        other = _frame(t, f"index-swapped-table-{residence}-{name}", integ, True)
        n_diff = int((other[0].view(np.uint32) != first[name][0].view(np.uint32)).any(axis=-1).sum())
        print(f"{residence} {name}: the table's entries alone swapped: {n_diff} pixels differ")
        assert n_diff > 0
    # ... with the two material records and the two indices of the triangle array swapped as well: the same picture
    v2 = _with_materials(s, extra=2)
    for i in range(v.n_material):
        v2.materials[i] = v.materials[i]
    v2.materials[a], v2.materials[b] = v.materials[b], v.materials[a]
    tri2 = tri.copy()
    tri2[tri == a], tri2[tri == b] = b, a
    _upload(t, s, view=v2, tri=tri2)
    t.seed(SEED)                            # (trc_resize left the RNG texture zero: nothing may launch on it, refused or not)
    _refused(lambda: t.render(spp=SPP, integrator=lc.PATH, material_params=True), abi.ERR_UNSUPPORTED)        # the upload dropped the table
    t.upload_material_params(swapped)
    for name, integ in INTEGRATORS.items():
        _same(_frame(t, f"index-swapped-all-{residence}-{name}", integ, True), first[name], f"{residence} {name}: records, entries and indices swapped")


# ---------------------------------------------------------------------- 6. the parameters act
def _primary_materials(t, s):
    rays = host.generate_camera_rays(s.cam, W, H)[0]
    hits = t.trace_rays(np.ascontiguousarray(rays.ravel()), production=True)
    return np.where(hits["hit"] != 0, hits["material"].astype(np.int64), -1).reshape(H, W)


@pytest.mark.parametrize("residence", ("lds", "mem"))
def test_the_parameters_reach_the_picture(rgpu, residence):
    t, s = rgpu, lc.cornell(residence, False, False)
    _upload(t, s)
    types = np.array(_types(s.view))
    try:
        first_hit = _primary_materials(t, s)
    except TracerError:
        FAULTED.append("act-trace")
        raise
    t.upload_material_params(_defaults(s.view))
    base = {name: _frame(t, f"act-base-{residence}-{name}", integ, True) for name, integ in INTEGRATORS.items()}
    for mtype, label, change in ((abi.MAT_METAL, "Metal at (0.3, 0.3)", dict(alpha_x=0.3, alpha_y=0.3)), (abi.MAT_GLASS, "Glass at eta 1.3", dict(eta=1.3))):
        table = _defaults(s.view)
        for field, value in change.items():
            table[field][types == mtype] = value
        t.upload_material_params(table)
        on = np.isin(first_hit, np.flatnonzero(types == mtype))
        assert on.sum() >= 20, (label, int(on.sum()))
        for name, integ in INTEGRATORS.items():
            got = _frame(t, f"act-{residence}-{name}-{label}", integ, True)
            assert np.isfinite(got[0]).all()
            changed = (got[0].view(np.uint32) != base[name][0].view(np.uint32)).any(axis=-1)
            print(f"{residence} {name} {label}: {int(changed[on].sum())} of {int(on.sum())} pixels whose camera ray hits it changed, {int(changed[~on].sum())} others")
            # The frame changes on those pixels.  How many of them is no property of the feature: under tracePath with a constant environment
            # a sample's radiance is the product of the colours it met -- Russian roulette divides the throughput by its own luminance, so
            # the scalar part of a lobe's f / pdf cancels, and a Lambert bounce contributes its colour alone -- times the constant, whatever
            # the directions were.  Another index bends the path; where it still meets the same materials the pixel keeps its bits
            # (measured: 141 of 292 glass pixels change on the tree in LDS, 128 of 257 on the tree read from memory, and 63 of the
            # unchanged ones are not black; all 138 metal pixels change, under both integrators).
            assert changed[on].sum() > 0, (label, name)
    # ... and the defaults again give the first frames again: nothing of a table outlives it
    t.upload_material_params(_defaults(s.view))
    for name, integ in INTEGRATORS.items():
        _same(_frame(t, f"act-back-{residence}-{name}", integ, True), base[name], f"{residence} {name}: the default table again")
    # extreme but valid parameters: every frame stays finite
    table = mpl.random_params(np.random.RandomState(3), s.view.n_material)
    table["alpha_x"][::2], table["alpha_y"][1::2], table["eta"][::3] = 1e-6, 50.0, 1.0000001
    t.upload_material_params(table)
    for name, integ in INTEGRATORS.items():
        assert np.isfinite(_frame(t, f"act-extreme-{residence}-{name}", integ, True)[0]).all()


def test_a_lambert_scene_reads_no_parameter(rgpu):
    t, s = rgpu, lc.cornell("lds", False, True)
    v = _with_materials(s)
    for i in range(v.n_material):
        if v.materials[i].type in (abi.MAT_PLASTIC, abi.MAT_METAL, abi.MAT_GLASS):
            v.materials[i].type = abi.MAT_LAMBERT
    _upload(t, s, view=v)
    t.upload_material_params(mpl.random_params(np.random.RandomState(4), v.n_material))
    for name, integ in INTEGRATORS.items():
        want = _frame(t, f"lambert-{name}", integ, False)
        _same(_frame(t, f"lambert-flagged-{name}", integ, True), want, f"Lambert-only scene, {name}, a random table")
        assert t.last_material_params()


# ---------------------------------------------------------------------- 7. composition
def test_tile_mask_tile_ranks_and_adaptive_passes(rgpu):
    t, s = rgpu, lc.cornell("mem", False, True)
    _upload(t, s)
    table = mpl.random_params(np.random.RandomState(5), s.view.n_material)
    t.upload_material_params(table)
    whole = _frame(t, "compose-whole", lc.MIS, True)
    assert t.last_material_params()
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
    try:
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        for rank in (0, 1):                                   # two tile ranks assemble the whole frame
            t.render(spp=SPP, integrator=lc.MIS, tile_rank=rank, tile_nranks=2, material_params=True)
            assert t.last_material_params()
        st = t.stats()
        _same((t.download_accum(), t.download_rng(), (st.rays, st.paths, st.shaded)), whole, "compose-ranks")
        t.seed(SEED); t.clear_accum(); t.reset_stats()
        rep = t.render_adaptive(threshold=0.05, max_spp=32, spp=8, integrator=lc.MIS, flags=abi.FLAG_MATERIAL_PARAMS)
        assert t.last_material_params()
        paths = t.stats().paths
        print(f"adaptive: {rep.as_dict()}, paths {paths}")
        assert rep.passes >= 2 and rep.samples == paths and N * 16 <= paths <= N * 32
        assert np.isfinite(t.download_accum()).all()
    except TracerError:
        FAULTED.append("compose")
        raise


# ---------------------------------------------------------------------- 8. refusals and lifetime
def test_refusals_and_lifetime(rgpu):
    t, s = rgpu, lc.cornell("lds", False, True)
    _upload(t, s)
    nm = s.view.n_material
    t.seed(SEED); t.clear_accum()
    before = t.download_accum(), t.download_rng()

    def unchanged():
        assert np.array_equal(u32(t.download_accum()), u32(before[0])) and np.array_equal(t.download_rng(), before[1])
    flagged = lambda **kw: t.render(**{**dict(spp=SPP, integrator=lc.MIS, material_params=True), **kw})
    _refused(flagged, abi.ERR_UNSUPPORTED)                                                   # the flag without a table
    _refused(lambda: t.download_material_params(nm), abi.ERR_INVALID_ARG)
    table = mpl.random_params(np.random.RandomState(6), nm)
    t.upload_material_params(table)
    assert t.download_material_params(nm).tobytes() == table.tobytes()
    # a refused upload changes nothing: every invalid field, a wrong count, NULL with a count
    for field, values in (("alpha_x", (0.0, -0.1, np.nan, np.inf)), ("alpha_y", (0.0, -1.0, np.nan)), ("eta", (1.0, 0.5, -2.0, np.nan, np.inf)),
                          ("metal_eta", (0.0, -1.0, np.nan, np.inf)), ("metal_k", (0.0, -0.5, np.nan, -np.inf))):
        for value in values:
            bad = table.copy()
            if field.startswith("metal"):
                bad[field][nm // 2, 1] = value
            else:
                bad[field][nm - 1] = value
            _refused(lambda: t.upload_material_params(bad), abi.ERR_INVALID_ARG)
    _refused(lambda: t.upload_material_params(table[:-1].copy()), abi.ERR_INVALID_ARG)
    _refused(lambda: t.upload_material_params(np.concatenate([table, table[:1]])), abi.ERR_INVALID_ARG)
    L, h = t._L, t._h
    assert L.trc_upload_material_params(h, None, nm) == abi.ERR_INVALID_ARG and L.trc_upload_material_params(h, table.ctypes.data, 0) == abi.ERR_INVALID_ARG
    assert L.trc_download_material_params(h, None, nm) == abi.ERR_INVALID_ARG
    _refused(lambda: t.download_material_params(nm + 1), abi.ERR_INVALID_ARG)
    assert t.download_material_params(nm).tobytes() == table.tobytes()
    # refused renders: nothing rendered, accumulator, RNG texture and table as they were
    _refused(lambda: flagged(integrator=lc.VOLUME), abi.ERR_UNSUPPORTED)
    t.generate_camera_rays(abi.RAYS_PINHOLE, 1, None)
    t.set_environment_map(lc.env_map("sun"))
    for kw in (dict(sobol=True), dict(collect_stats=True), dict(env_light=True), dict(mesh_lights=True), dict(camera_rays=True), dict(view_height=15)):
        _refused(lambda: flagged(**kw), abi.ERR_UNSUPPORTED)
    t.set_environment_map(None); t.clear_camera_rays()
    _refused(lambda: t.render_adaptive(threshold=0.05, max_spp=32, spp=8, integrator=lc.VOLUME, flags=abi.FLAG_MATERIAL_PARAMS), abi.ERR_UNSUPPORTED)
    unchanged()
    assert t.download_material_params(nm).tobytes() == table.tobytes()
    try:
        want = _frame(t, "life-first", lc.MIS, True)
        # the calls that keep the table: animation, a rebuilt tree, visibility, per-triangle materials, textures, trc_resize
        verts = t.download_vertices()
        t.update_vertices(verts)
        t.rebuild_tree(0)
        t.set_triangle_visibility([(0, 1, 1)])
        t.upload_triangle_materials(s.tri); t.upload_textures([]); t.resize(W, H); t.seed(SEED)
        assert t.download_material_params(nm).tobytes() == table.tobytes()
        flagged()
        assert t.last_material_params()
        # the scene as it was uploaded: the same picture as before those calls
        t.upload_scene(s.view)
        _refused(flagged, abi.ERR_UNSUPPORTED)                                               # every scene upload drops the table
        _refused(lambda: t.download_material_params(nm), abi.ERR_INVALID_ARG)
        t.upload_triangle_materials(s.tri)
        t.upload_material_params(table)
        _same(_frame(t, "life-again", lc.MIS, True), want, "the same table on the same scene again")
        t.upload_material_params(None)                                                       # (NULL, 0): none in force
        _refused(flagged, abi.ERR_UNSUPPORTED)
        plain = _frame(t, "life-plain", lc.MIS, False)
        assert not t.last_material_params() and np.isfinite(plain[0]).all()
    except TracerError:
        FAULTED.append("lifetime")
        raise
    with Tracer(0, hooks=True) as fresh:                                                     # no scene
        assert fresh._L.trc_upload_material_params(fresh._h, table.ctypes.data, nm) == abi.ERR_NO_SCENE
