"""trc_debug_set and the knobs' defaults (tracer_abi.h): every knob name is accepted, an unknown one is refused and leaves the context
as it was, negative values clamp to 0, and trc_create reads the defaults from the environment.  Knobs are scheduling only, so every
frame compared here is compared bit for bit.  The frames of this module run kernels that keep no primary-replay memo: replay_min_lanes
and replay_chain are only named here, and are run with values, on the kernels that have a memo, by the replay matrix of
tests/test_gpu_primary_replay.py (test_replay_schedule_knobs_change_nothing).  The module renders on hooks Tracers of its own
(trc_debug_last_kernel)."""
import os

import numpy as np
import pytest

from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu

# the names trc_debug_set knows, spelled out: a knob that drops out of the library's table fails here by name
KNOBS = ["no_lds_fit", "stack_lds_levels", "strip_len", "no_pwg", "sppm_serial_camera", "sppm_timing", "force_blk_shift", "no_split",
         "no_cost_filter", "no_cold_probe", "probe_spp", "no_plan_reuse", "no_coalesce", "no_dense", "head_stages", "descend_min",
         "camera_policy", "no_primary_replay", "replay_min_lanes", "replay_chain", "mesh_light_pick", "refit_single", "strip_force"]
W, H = 32, 32          # 16 blocks of 8 x 8
SEED = 7


def _cornell(t, scene, w, h):
    t.upload_scene(scene.view)
    t.set_camera(host.prepare_camera(w, h))
    t.set_environment((0.0, 0.0, 0.0))
    t.resize(w, h)


def _frame(t, spp):
    """a tracePath frame from a fresh seed -> (accumulator bits, RNG texture, kernel choice)"""
    t.seed(SEED); t.clear_accum()
    t.render(spp=spp, integrator=abi.INTEGRATOR_PATH)
    return t.download_accum().view(np.uint32), t.download_rng(), t.last_kernel()


@pytest.fixture(scope="module")
def cornell():
    return host.HostScene(abi.SCENE_CORNELL)


@pytest.fixture(scope="module")
def kgpu(cornell):
    t = Tracer(0, hooks=True)
    _cornell(t, cornell, W, H)
    yield t
    t.close()


@pytest.mark.parametrize("name", KNOBS)
def test_every_knob_name_is_accepted(kgpu, name):
    kgpu.debug_set(name, 0)
    if name == "mesh_light_pick":
        kgpu.debug_set(name, 1)         # its default


def test_unknown_name_is_refused_and_changes_nothing(kgpu, cornell):
    name = "no_such_knob"
    with pytest.raises(TracerError) as err:
        kgpu.debug_set(name, 1)
    assert err.value.status == abi.ERR_INVALID_ARG
    assert name in str(err.value)
    accum, rng, _ = _frame(kgpu, 4)
    with Tracer(0, hooks=True) as fresh:                     # a context that never saw the refusal
        _cornell(fresh, cornell, W, H)
        accum_ref, rng_ref, _ = _frame(fresh, 4)
    assert np.array_equal(accum, accum_ref) and np.array_equal(rng, rng_ref)


def test_negative_values_clamp_to_zero(kgpu):
    kgpu.debug_set("strip_force", 2)
    try:
        assert _frame(kgpu, 1)[2]["strip"] == 2
        kgpu.debug_set("strip_force", -5)                    # 0: the launch geometry's own choice, one block per wavefront on 16 blocks
        assert _frame(kgpu, 1)[2]["strip"] == 1
    finally:
        kgpu.debug_set("strip_force", 0)


def test_environment_defaults_are_read_at_create():
    """Cornell + Mesh.ball(24, 24, 1.0) (the 'bigball' of test_gpu_mesh_lights.py: 1152 triangles, 1104 of them with area; the tree is read
    from memory, asserted below), 96 x 64 at 8 spp, tracePath: persistent workgroups
    by default, one block per one-wavefront workgroup under TRC_NO_PWG=1; knob no_pwg = 0 brings them back; the same frame each time."""
    scene = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(24, 24, 1.0))
    assert scene.view.n_index // 3 == 1152
    before = os.environ.get("TRC_NO_PWG")
    with Tracer(0, hooks=True) as plain:
        _cornell(plain, scene, 96, 64)
        accum, rng, kern = _frame(plain, 8)
    assert kern["shape"] == "pwg" and not kern["lds_resident"]
    os.environ["TRC_NO_PWG"] = "1"
    try:
        knobbed = Tracer(0, hooks=True)
    finally:
        if before is None:
            del os.environ["TRC_NO_PWG"]
        else:
            os.environ["TRC_NO_PWG"] = before
    with knobbed:
        _cornell(knobbed, scene, 96, 64)
        accum_one, rng_one, kern_one = _frame(knobbed, 8)
        assert kern_one["shape"] == "one"
        knobbed.debug_set("no_pwg", 0)
        accum_back, rng_back, kern_back = _frame(knobbed, 8)
        assert kern_back["shape"] == "pwg"
    assert np.array_equal(accum, accum_one) and np.array_equal(rng, rng_one)
    assert np.array_equal(accum, accum_back) and np.array_equal(rng, rng_back)
