"""The CPU oracle held to the reference's own shader text, bit for bit (CPU only).

oracle/_ref/libmetal_ref.so is RT_Metal/Metal/*.hh compiled on the host against oracle/metal_shim/metal_stdlib (oracle/Makefile,
oracle/ref_metal_entry.cpp); every ref_* entry point has an orc_* twin of the same signature over the oracle's restatement
(oracle/pin_api.h).  Two sets of tests over the same inputs (tests/reference_pin_cases.py):

  live    ref_* against orc_*, skipped where the reference (and so the library) is absent;
  golden  orc_* against what ref_* answered when tests/golden/make_reference_pin.py last ran, never skipped.

Each function gets hand-made edge inputs and 200 000 seeded ones; all NaNs count as equal.  Edge classes:
  sphere    discriminant exactly 0 and +-1..3 ulp; near / far root exactly t_min / t_max and 1 ulp off; origin inside and on the
            surface; a denormal, direction not normalised; radius inflated by 1e-4; gn.y = +-1 with gn.x = gn.z = +-0; grazing rays
  square    all three axes; direction[k] = +-0 and denormal, with the origin on and off the plane; t exactly range_t.x / .y; a, b
            on each edge and 1 ulp outside; the corners; signed zeros; both faces; origin on the plane; a dyadic grid of rays
  triangle  fabs(det) exactly FLT_EPSILON and +-1, 2 ulp; u, v, u + v exactly 0 / 1 and 1 ulp beyond; t == range.x / .y; zero-area and
            sliver triangles; back-facing; vertex normals not normalised; a dyadic grid; rays nearly in the triangle's plane
  cube      origin inside, outside, exactly on a face; direction components +-0, denormal; scaled and rotated model matrices; te
            crossing tmax around te * (1 + 2 gamma(3)); _record.t >= range_t.y with equality; rays through edges and corners
  AABB      tmax < 0; tmin < 0 <= tmax; zero-thickness and point boxes; rays in a face plane (0 * inf); range_t.x = FLT_MIN
  Scene::hit  cornell_spheres, ball_mesh_scene, adversarial_scene seeds 1-6; closest and any-hit, tmax == t and 1 ulp either side
  lobes     every material type of the ABI (+ a checker texture, + types without a lobe); wo.z, wi.z = +-0, grazing 1e-4, wo == wi,
            wo == -wi, the mirror direction, wrong hemisphere, non-unit and null vectors; uu in {0, 1, 1 - 2^-24, 0.5, 0.25 +- 1 ulp};
            Beckmann / TrowbridgeReitz alphas 1e-3 (EffectivelySmooth), below it, 1; Fresnel and Refract with eta = 1 and around the
            critical angle (+-50 ulp)
  math      offset_ray with |p| < 1/32, exactly +-1/32 and 1 ulp off, p = +-0, negative; ErfInv at +-0.99999 and +-200 ulp around
            w == 5; NextFloatUp / Down at +-0, +-inf, denormals, +-FLT_MAX, NaN

Fields the reference leaves unwritten (UNWRITTEN below) are indeterminate in its host build and 0 in the oracle (its B-3 convention).
They are excluded by field per primitive type, never by input; the table was checked by hand against the reference's text
(ASSIGNED lists, per hit_test, the fields it assigns and where), and the tests assert that the two are disjoint, that together
they are the whole record, and that every other field is compared for every input.
"""
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT
from oracle import pyoracle as po
import reference_pin_cases as rc

# field -> where the reference assigns it; a field of pin_rec that is not here is one the hit_test never writes
ASSIGNED = {
    "sphere": {"t": "Sphere.hh:51,65", "p": "Sphere.hh:52,66", "gn": "Sphere.hh:53,67", "sn": "HitRecord.hh:28 via Sphere.hh:54,68",
               "f": "HitRecord.hh:27", "uv": "Sphere.hh:55,69", "material": "Sphere.hh:56,70", "range_y": "Sphere.hh:58,72"},
    "square": {"uv": "Square.hh:93-94", "t": "Square.hh:96", "gn": "Square.hh:98-101", "sn": "HitRecord.hh:28 via Square.hh:100",
               "f": "HitRecord.hh:27", "p": "Square.hh:104-106", "range_y": "Square.hh:108", "PDF": "Square.hh:109", "material": "Square.hh:110"},
    "triangle": {"p": "Triangle.hh:73", "range_y": "Triangle.hh:75", "t": "Triangle.hh:76", "gn": "Triangle.hh:78", "uv": "Triangle.hh:79",
                 "sn": "HitRecord.hh:28 via Triangle.hh:81", "f": "HitRecord.hh:27", "material": "Triangle.hh:82"},
    # Cube::hit_test fills a LOCAL `HitRecord _record;` (Cube.hh:22) and copies it whole (Cube.hh:45): what it never assigns is garbage
    "cube": {"t": "AABB.hh:149,192 then Cube.hh:32", "gn": "AABB.hh:151-152,194-195 then Cube.hh:42", "p": "AABB.hh:155-157,198-200 then Cube.hh:27",
             "uv": "AABB.hh:163,206", "range_y": "Cube.hh:36", "material": "Cube.hh:38", "sn": "HitRecord.hh:28 via Cube.hh:43", "f": "HitRecord.hh:27"},
    "aabb_record": {"t": "AABB.hh:149,192", "gn": "AABB.hh:151-152,194-195", "p": "AABB.hh:155-157,198-200", "uv": "AABB.hh:163,206"},
}
UNWRITTEN = rc.EXCLUDED            # {"sphere": {"PDF"}, "square": {}, "cube": {"PDF"}, "triangle": {"PDF"}, "aabb_record": {"sn", "f", "material", "PDF"}}
# Scene::hit (Render.hh:135-252) hands ONE record to every leaf it tests: after a cube was accepted its PDF is that cube's garbage
# (Cube.hh:22,45) whatever wins later, and nothing in the record says whether the walk met a cube.  range_y is not Scene::hit's.
SCENE_UNWRITTEN = rc.SCENE_EXCLUDED

LIVE = os.path.exists(po.METAL_REF)
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_pin.npz"))
CASES = rc.build_cases()
_BITS = {}


def orc_bits(name):
    """the oracle's answer to a case, computed once for both sets of tests"""
    if name not in _BITS:
        case = CASES[name]
        fields = case.run(po.Pin())
        compared = [f for f in fields if f not in case.excluded]
        assert set(compared) | set(case.excluded) >= set(fields) and compared, name
        bits = rc.canonical(fields, case.excluded)
        width = sum(int(np.prod(np.shape(fields[f])[1:])) for f in compared)
        assert bits.shape == (len(next(iter(fields.values()))), width), "every field outside the table is compared for every input"
        _BITS[name] = (bits, fields)
    return _BITS[name]


def first_difference(a, b):
    bad = np.argwhere((a != b).any(1))
    return f"{len(bad)} of {len(a)} inputs differ, first at input {bad[0][0]}: {a[bad[0][0]]} != {b[bad[0][0]]}" if len(bad) else ""


def test_the_table_of_unwritten_fields_names_no_field_a_hit_test_assigns():
    record = set(rc.REC_FIELDS) - {"accepted"}
    for prim, unwritten in UNWRITTEN.items():
        assert not (set(unwritten) & set(ASSIGNED[prim])), prim
        assert set(unwritten) | set(ASSIGNED[prim]) | ({"range_y"} if prim == "aabb_record" else set()) == record, prim
        assert CASES[prim].excluded == frozenset(unwritten)
    for name, case in CASES.items():
        if name.startswith("scene_"):
            assert case.excluded == frozenset(SCENE_UNWRITTEN)
        elif name not in UNWRITTEN:
            assert not case.excluded, name


def test_every_case_has_its_edges_and_200000_seeded_inputs():
    for name, case in CASES.items():
        n = len(orc_bits(name)[0])
        if name.startswith("scene_"):
            assert n == rc.N_SCENE_RAYS
        elif name != "gamma":
            assert n >= case.n_edge + rc.N_SEEDED, name
    for prim in ("sphere", "square", "triangle", "cube", "aabb_record"):      # neither all hits nor all misses, edges included
        acc = orc_bits(prim)[1]["accepted"]
        stored = CASES[prim].stored[:-rc.N_STORED]
        assert 0.1 < (acc[stored] != 0).mean() < 0.9 and 0.1 < (acc[CASES[prim].n_edge:] != 0).mean() < 0.9, prim


# ----------------------------------------------------------------------------------------------------------------- live
needs_reference = pytest.mark.skipif(not LIVE, reason="oracle/_ref/libmetal_ref.so not built (the reference is not on this machine)")


@needs_reference
def test_live_the_reference_library_reads_literals_as_float():
    """1.0 - u - v (Triangle.hh:68) is two float subtractions in MSL; computed in double and rounded once it differs here"""
    u, v = np.float32(0.1), np.float32(0.7)
    two_float_subtractions = np.float32(np.float32(1.0) - u) - v
    assert np.float32(1.0 - float(u) - float(v)) != two_float_subtractions           # the input tells the two routes apart
    assert po.Pin(ref=True).literal_probe(u, v) == two_float_subtractions
    assert po.Pin().literal_probe(u, v) == two_float_subtractions


@needs_reference
@pytest.mark.parametrize("name", list(CASES))
def test_live_oracle_matches_the_reference_headers(name):
    case = CASES[name]
    ref = rc.canonical(case.run(po.Pin(ref=True)), case.excluded)
    orc = orc_bits(name)[0]
    assert ref.shape == orc.shape
    assert not (ref != orc).any(), f"{name}: " + first_difference(orc, ref)


# ----------------------------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("name", list(CASES))
def test_golden_oracle_matches_the_recorded_reference(name):
    case = CASES[name]
    orc = orc_bits(name)[0]
    assert len(orc) == int(GOLDEN[f"n/{name}"])
    head, stored = GOLDEN[f"head/{name}"], case.stored[case.stored < len(orc)]
    assert head.shape == orc[stored].shape
    assert not (head != orc[stored]).any(), f"{name}, among the recorded outputs: " + first_difference(orc[stored], head)
    assert zlib.crc32(orc.tobytes()) == int(GOLDEN[f"crc/{name}"]), f"{name}: the CRC-32 over all {len(orc)} inputs differs (recorded outputs agree)"


@pytest.mark.parametrize("name", rc.GPU_SCENES)
def test_golden_trace_rays_of_the_oracle_matches_the_recorded_scene_hit(name):
    """orc_trace_rays is what the GPU tests hold trc_trace_rays to: its trc_hit records against the reference's own walk"""
    sv, _, rays = rc._scene_views()[name]
    closest = po.trace_rays(sv, rays)
    bits = rc.canonical(rc.trc_view(closest["hit"], closest))
    assert zlib.crc32(bits.tobytes()) == int(GOLDEN[f"crc/trc/{name}"]), name
    shadow = po.trace_rays(sv, rc.shadow_rays(name, rays, closest["t"], closest["hit"]), any_hit=True)
    assert zlib.crc32(rc.canonical(rc.trc_view(shadow["hit"], shadow)).tobytes()) == int(GOLDEN[f"crc/trc_any/{name}"]), name
    assert 0.05 < (shadow["hit"] != 0).mean() < 0.95
