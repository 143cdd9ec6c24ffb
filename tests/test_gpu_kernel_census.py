"""A census of the render kernel tables: every entry of render_kernels<LDS, INTEGRATOR>(), of its per-triangle-material twin (namespace
trimat: separate kernels) and k_render_dense of both families is launched through the C ABI, named by trc_debug_last_kernel, and
held to the oracle -- accumulator bits, RNG texture, rays / paths / shaded, and under TRC_FLAG_COLLECT_STATS every traversal counter.

The enumeration (light_oracle_cases.table_entries) is built from abi.KERNEL_VARIANTS x abi.KERNEL_SHAPES x the three integrators by
the rule of render_kernels(): a variant or a shape added to the library shows here as unreached.  The light variants of both families
and the Tex entries of the plain one are asserted by tests/test_gpu_light_oracle.py: its cases count here (rendered through its
cache, so once per run); every other entry has a case of its own below -- Cornell + the 48-triangle ball (the tree in LDS) or the
1104-triangle one (read from memory), random per-triangle materials in the trimat family, 61 x 45, a constant environment that is
not black, 8 samples (the fewest of a whole-block launch) or 2 under knob strip_force, knob no_pwg for `one` on a tree read from
memory.  The dense entries take a frame of the smallest class the criterion admits, compared on one tile in 64.

Like test_gpu_light_oracle.py, whose launch and check it shares: after a TracerError nothing more of these modules is asked of the GPU."""
import numpy as np
import pytest

import light_oracle_cases as lc
import test_gpu_light_oracle as tlo
from oracle import pyoracle as po
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu

CASES = lc.census_cases()
DENSE_W, DENSE_H, DENSE_SPP, DENSE_NRANKS = 1916, 1076, 8, 64
_DENSE = {}                  # family -> the entry its dense launch took


@pytest.fixture(scope="module")
def cgpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_entry_matches_the_oracle(cgpu, case):
    got = tlo._render_case(cgpu, case)
    assert tlo._entry(case, got[3]) == case.entry, got[3]
    tlo._check(case, got)


def _dense(t, family):
    """one 1916 x 1076 launch of 8 samples on the 12-triangle ball (light_oracle_cases.cornell: the largest mesh whose workgroups the
    dense kernel is given), every triangle material 19 or a random one; the oracle renders one tile in 64 of it"""
    if family not in _DENSE:
        if tlo.FAULTED:
            pytest.fail(f"not run: {tlo.FAULTED[0]} left an error on the device")
        s = lc.cornell("tiny", False, family == "trimat")
        cam = host.prepare_camera(DENSE_W, DENSE_H)
        try:
            t.upload_scene(s.view); t.upload_triangle_materials(s.tri); t.upload_textures([])
            t.set_camera(cam); t.set_environment(lc.ENV_RGB); t.set_environment_map(None); t.resize(DENSE_W, DENSE_H)
            t.seed(lc.SEED); t.clear_accum(); t.reset_stats()
            t.render(spp=DENSE_SPP, integrator=lc.PATH)
            acc, rng, st, k = t.download_accum(), t.download_rng(), t.stats(), t.last_kernel()
            t.set_environment((0.0, 0.0, 0.0)); t.resize(lc.W, lc.H)
        except TracerError:
            tlo.FAULTED.append(f"dense-{family}")
            raise
        ref_rng = host.fill_rng(lc.SEED, DENSE_W, DENSE_H)
        ref, ref_st = po.render(s.view, cam, DENSE_W, DENSE_H, ref_rng, spp=DENSE_SPP, integrator=lc.PATH, env=lc.ENV_RGB, triangle_materials=s.tri,
                                tile_rank=0, tile_nranks=DENSE_NRANKS)
        _DENSE[family] = (acc, rng, st, k, ref, ref_rng, ref_st)
    return _DENSE[family]


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_dense_entry_matches_the_oracle(cgpu, family):
    acc, rng, st, k, ref, ref_rng, ref_st = _dense(cgpu, family)
    ty, tx = np.mgrid[0:DENSE_H, 0:DENSE_W] // abi.TRC_TILE
    mine = ((tx + ty) % DENSE_NRANKS) == 0
    print(f"dense-{family}: kernel {k}; {int(mine.sum())} pixels compared")
    assert k["shape"] == "dense" and k["variant"] == "plain" and k["lds_resident"] and k["triangle_materials"] == (family == "trimat"), k
    assert mine.sum() > 5000 and st.paths == DENSE_W * DENSE_H * DENSE_SPP and ref_st.paths == mine.sum() * DENSE_SPP
    assert np.isfinite(acc).all()
    assert np.array_equal(acc[mine].view(np.uint32), ref[mine].view(np.uint32))
    assert np.array_equal(rng[mine], ref_rng[mine])


def test_every_entry_of_the_kernel_tables_was_reached(cgpu):
    """want <= reached over the whole enumeration.  What an earlier test of the run rendered is taken from the cache; a run of this
    test alone renders everything (the kernel choice is read from the launch itself, never from the case's wish)."""
    reached = {}
    for c in tlo.MATRIX + tlo.BEYOND + CASES:
        reached.setdefault(tlo._entry(c, tlo._render_case(cgpu, c)[3]), c.id)
    for family in lc.FAMILIES:
        k = _dense(cgpu, family)[3]
        reached.setdefault((lc.FAMILIES[k["triangle_materials"]], lc.PATH, k["variant"], "lds" if k["lds_resident"] else "mem", k["shape"]), f"dense-{family}")
    want = set(lc.table_entries())
    for e in sorted(want):
        print(e[0], lc.INTEGRATOR_NAMES[e[1]], *e[2:], "<-", reached.get(e, "NOT REACHED"))
    missing = sorted(want - set(reached))
    print(f"{len(want)} entries, {len(missing)} not reached")
    assert not missing, missing
    assert set(abi.KERNEL_VARIANTS) == {e[2] for e in want} and set(abi.KERNEL_SHAPES) == {e[4] for e in want}
