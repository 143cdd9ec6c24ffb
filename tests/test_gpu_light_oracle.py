"""The render kernels against the oracle on the project's own four features (per-triangle materials, image textures,
TRC_FLAG_ENV_LIGHT, TRC_FLAG_MESH_LIGHTS; oracle/README.md): every case renders one 61 x 45 frame on the GPU and in the oracle and
compares the accumulator's bits, the RNG texture and the rays / paths / shaded counters, and asserts through trc_debug_last_kernel
that the kernel it was written for ran.  The cases (tests/light_oracle_cases.py) cover every Env, EnvTex, Mesh and MeshTex entry of the
kernel tables and of their per-triangle-material twins, both tree residences; tests/test_oracle_lights.py shows that they reach every branch of the light code.  Strip launches
are forced with knob strip_force (a frame of 48 blocks never gets a strip otherwise)."""
import numpy as np
import pytest

import light_oracle_cases as lc
from conftest import camera_rays
from oracle import pyoracle as po
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError
from test_gpu_primary_replay import STAT_FIELDS

pytestmark = pytest.mark.gpu
W, H = lc.W, lc.H
_GOT = {}                   # case id -> what the GPU gave: a case renders once, whichever test asks first
FAULTED = []                # the case whose launch left an error behind: nothing more of this module runs on the GPU after it
FAMILIES = {False: "plain", True: "trimat"}


@pytest.fixture(scope="module")
def lgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def _upload(t, s, env=None, env_rgb=(0.0, 0.0, 0.0), cam=None):
    t.upload_scene(s.view)
    t.upload_triangle_materials(s.tri)
    t.upload_textures(s.images)
    t.set_camera(cam if cam is not None else s.cam); t.set_environment(env_rgb); t.resize(W, H)
    t.set_environment_map(lc.env_map(env) if env else None)
    t.seed(lc.SEED); t.clear_accum(); t.reset_stats()


def _render_case(t, case):
    """the case on the GPU -> (accum, rng, stats, kernel choice)"""
    if case.id not in _GOT:
        if FAULTED:
            pytest.fail(f"not run: {FAULTED[0]} left an error on the device")
        try:
            _GOT[case.id] = _launch_case(t, case, case.scene)
        except TracerError:
            FAULTED.append(case.id)
            raise
    return _GOT[case.id]


def _launch_case(t, case, s):
    _upload(t, s, case.env, case.env_rgb, case.camera)
    t.debug_set("strip_force", 2 if case.shape == "strip" else 0)
    t.debug_set("no_pwg", 1 if case.shape == "one" else 0)
    t.debug_set("mesh_light_pick", case.pick)
    kw = dict(max_depth=case.max_depth, integrator=case.integrator, env_light=case.light == "env", mesh_lights=case.light == "mesh",
              sobol=case.sobol, collect_stats=case.stats)
    t.render(spp=case.spp, frame0=case.frame0, **kw)
    if case.second:
        t.render(spp=case.second, frame0=case.frame0 + case.spp, **kw)
    out = t.download_accum(), t.download_rng(), t.stats(), t.last_kernel()
    # (not in a `finally`: after a TracerError, a device fault included, nothing more is asked of this context)
    t.debug_set("strip_force", 0); t.debug_set("no_pwg", 0); t.debug_set("mesh_light_pick", 1)
    t.set_environment_map(None); t.upload_textures([]); t.set_environment((0.0, 0.0, 0.0))
    return out


def _entry(case, k):
    """the kernel-table entry a launch took: (family, integrator, variant, residence, shape)"""
    return (FAMILIES[k["triangle_materials"]], case.integrator, k["variant"], "lds" if k["lds_resident"] else "mem", k["shape"])


def _check(case, got):
    acc, rng, st, k = got
    ref_acc, ref_rng, ref_st = lc.oracle_frame(case)
    s = case.scene
    # (choose_kernel: a light, then images, then Sobol', then the counters)
    variant = (case.light + ("_tex" if s.images else "")) if case.light else ("tex" if s.images else "sobol" if case.sobol else "stats" if case.stats else "plain")
    print(f"{case.id}: kernel {_entry(case, k)}, strip {k['strip']}; "
          f"rays {st.rays} shaded {st.shaded}; accum mismatches {int((acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=-1).sum())}, "
          f"rng mismatches {int((rng != ref_rng).any(axis=-1).sum())}")
    assert k["shape"] == case.shape and k["variant"] == variant, k
    assert k["triangle_materials"] == (s.tri is not None) and k["strip"] == (2 if case.shape == "strip" else 1), k
    assert np.isfinite(acc).all()
    bad = np.argwhere((acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ, first (y, x) {bad[0]}: gpu {acc[tuple(bad[0])]} oracle {ref_acc[tuple(bad[0])]}"
    assert np.array_equal(rng, ref_rng)
    assert (st.rays, st.paths, st.shaded) == (ref_st.rays, ref_st.paths, ref_st.shaded)
    if case.stats:                               # TRC_FLAG_COLLECT_STATS: the traversal counters are the oracle's too
        for f in STAT_FIELDS:
            assert getattr(st, f) == getattr(ref_st, f), f


MATRIX, BEYOND = lc.matrix(), lc.beyond()
SHAPES = [(r, sh) for r in ("lds", "mem") for sh in ("one", "strip", "pwg") if (r, sh) != ("lds", "pwg")]      # an LDS-resident tree has no pwg kernel
LIGHT_VARIANTS = [v for v in abi.KERNEL_VARIANTS if v not in ("plain", "stats", "sobol", "tex")]                # a new variant lands here, unreached


@pytest.mark.parametrize("case", MATRIX, ids=repr)
def test_light_kernels_match_the_oracle(lgpu, case):
    got = _render_case(lgpu, case)
    assert got[3]["lds_resident"] == (case.id.split("-")[1] == "lds")
    _check(case, got)


def test_every_light_entry_of_the_kernel_tables_was_reached(lgpu):
    """every light variant the library knows (abi.KERNEL_VARIANTS: Env, EnvTex, Mesh, MeshTex) of render_kernels<LDS, MIS>(), in BOTH
    families -- the plain tables and their trimat twins, which are separate kernels --: `one` and `strip` on both residences, `pwg` on
    trees read from memory.  The matrix's cases are rendered here if no earlier test of the run did (a run of this test alone is whole)."""
    reached = {_entry(c, _render_case(lgpu, c)[3]) for c in MATRIX}
    want = {(f, lc.MIS, v, r, sh) for f in FAMILIES.values() for v in LIGHT_VARIANTS for (r, sh) in SHAPES}
    print("reached:", sorted(reached))
    assert len(LIGHT_VARIANTS) == 4 and want <= reached, sorted(want - reached)


@pytest.mark.parametrize("case", lc.further(), ids=repr)
def test_further_light_cases_match_the_oracle(lgpu, case):
    _check(case, _render_case(lgpu, case))


@pytest.mark.parametrize("case", BEYOND, ids=repr)
def test_triangle_materials_and_images_match_the_oracle(lgpu, case):
    _check(case, _render_case(lgpu, case))


def test_every_texture_entry_was_reached(lgpu):
    """the Tex entries of the three integrators' plain tables, one / strip / pwg on both residences (rendered here if not yet)"""
    reached = {_entry(c, _render_case(lgpu, c)[3]) for c in BEYOND}
    want = {("plain", i, "tex", r, sh) for i in (lc.PATH, lc.MIS, lc.VOLUME) for (r, sh) in SHAPES}
    assert want <= reached, sorted(want - reached)


def test_sppm_with_triangle_materials_matches_the_oracle(lgpu):
    """2 SPPM frames over random per-triangle materials: accumulator, canvas RNG, photon and camera records (test_generated_scene_sppm)"""
    s = lc.cornell("lds")
    t = lgpu
    _upload(t, s)
    t.sppm_init(77); t.sppm_frames(2)
    dcam, dpho, dmark, dcount, dcx = t.sppm_download()
    dacc, drng = t.download_accum(), t.download_rng()
    rng = host.fill_rng(lc.SEED, W, H); acc = np.zeros((H, W, 4), np.float32)
    o = po.Sppm(W, H, 77); o.frames(s.view, s.cam, rng, acc, 2, triangle_materials=s.tri)
    ocam, opho, omark, ocount, ocx = o.download()
    assert np.array_equal(drng, rng) and np.array_equal(dacc.view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(dcount, ocount) and np.array_equal(dmark, omark)
    for got, ref, fields in ((dpho, opho, ("flux", "normal", "position", "direction", "step", "active")),
                             (dcam, ocam, ("ratio", "position", "direction", "valid", "alternative", "flux", "radius", "photonCount"))):
        for f in fields:
            assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), f
    assert dcx.frame_count == ocx.frame_count and dcx.totalPhotonSum == ocx.totalPhotonSum


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_trace_rays_report_each_triangles_material(lgpu, residence):
    s = lc.cornell(residence)
    _upload(lgpu, s)
    rays = camera_rays(s.cam, 160, 120)
    dev = lgpu.trace_rays(rays)
    ref = po.trace_rays(s.view, rays, triangle_materials=s.tri)
    tri = (ref["hit"] != 0) & (ref["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 100 and len(np.unique(ref["material"][tri])) > 5
    for f in ("hit", "pType", "pIndex", "material"):
        assert np.array_equal(dev[f], ref[f]), f
    for f in ("t", "p", "gn", "sn", "uv", "PDF"):
        assert np.array_equal(dev[f].view(np.uint32), ref[f].view(np.uint32)), f
