"""trc_trace_rays held to the reference's OWN walk: the records that ref_scene_hit, Scene::hit of Render.hh:135-252 compiled on the
host from the reference's text (oracle/ref_metal_entry.cpp), returned for 8 192 rays per scene when
tests/golden/make_reference_pin.py last ran.  Not the oracle's records: the oracle is not consulted here, only tests/golden/.

The golden file holds the CRC-32 of all 8 192 records as trc_hit reports them (the answer, and t p gn sn uv material where the
answer is yes; PDF is not part of it: tests/test_reference_pin.py, SCENE_UNWRITTEN) and the first 512 records in full, which say
where a CRC went wrong.  The production walk of any-hit rays defines the answer alone (include/tracer_abi.h).
"""
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT
import reference_pin_cases as rc

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_pin.npz"))


def held(dev, name, key, what, fields=None):
    bits = rc.canonical(rc.trc_view(dev["hit"], dev))
    head = GOLDEN[f"head/scene_{key}{name}"]
    want = head[:, rc.TRC_VIEW_OF_SCENE_BITS].copy()
    want[want[:, 0] == 0, 1:] = 0                                   # the record only where the answer is yes
    cols = slice(0, 1) if fields == "hit" else slice(None)
    bad = np.argwhere((bits[:len(want), cols] != want[:, cols]).any(1))
    assert not len(bad), f"{what}: ray {bad[0][0]} is {bits[bad[0][0]]}, the reference's walk recorded {want[bad[0][0]]}"
    if fields == "hit":
        all_hits = GOLDEN[f"crc/hit_{key}{name}"]
        assert zlib.crc32(np.ascontiguousarray(bits[:, 0]).tobytes()) == int(all_hits), f"{what}: answers beyond the first {len(want)} rays differ"
    else:
        assert zlib.crc32(bits.tobytes()) == int(GOLDEN[f"crc/trc{'_any' if key else ''}/{name}"]), f"{what}: records beyond the first {len(want)} rays differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.GPU_SCENES)
def test_trace_rays_matches_the_recorded_walk_of_the_reference(gpu, name):
    sv, keep, rays = rc._scene_views()[name]
    gpu.upload_scene(sv)
    closest = gpu.trace_rays(rays)
    held(closest, name, "", f"{name}, closest, instrumented")
    held(gpu.trace_rays(rays, production=True), name, "", f"{name}, closest, production")
    shadow = rc.shadow_rays(name, rays, closest["t"], closest["hit"])             # tmax == t of the closest hit among them
    held(gpu.trace_rays(shadow, any_hit=True), name, "any_", f"{name}, any-hit, instrumented")
    held(gpu.trace_rays(shadow, any_hit=True, production=True), name, "any_", f"{name}, any-hit, production", fields="hit")
