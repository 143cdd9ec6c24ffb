"""The host side of the camera-ray sets (include/tracer_abi.h "Camera-ray sets"): trc_host_generate_camera_rays against a float64 restatement
of the three models, its pinhole rays at zero offset against castRay's own binary32 expression, trc_host_halton_offsets against exact
fractions, and the argument errors.  No GPU: tests/test_gpu_camera_rays.py holds the device generator to this one bit for bit.

Bounds.  Pinhole and orthographic: origin and (unnormalised) direction are sums of three products and one or two differences in binary32, and
s, t carry one rounding each; every rounding is at most half an ulp of its result, and every result is bounded by the largest-magnitude
operand of its sum up to a factor 2: 4 ulp of the largest operand, per component.  Equirectangular: unit vectors from two dm_ calls of
stated accuracy (a few ulp at most 1) and one product: 1e-6 absolute."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import camera_rays
from tracer_amd import abi, host

F = np.float32
FLT_MAX = np.finfo(F).max
SIZES = ((61, 45), (1, 1), (7, 3), (128, 96))


def cameras(w, h):
    yield "prepare", host.prepare_camera(w, h)
    yield "off-axis", host.make_camera((500.0, 40.0, -450.0), (200.0, 450.0, 250.0), (0.0, 1.0, 0.0), 0.0, w / h, float(np.deg2rad(50.0)), 10.0)
    yield "near", host.make_camera((-3.5, 0.25, 7.0), (0.125, -1.0, 0.5), (0.1, 1.0, 0.0), 0.0, w / h, float(np.deg2rad(25.0)), 2.5)


def vec(a):
    return np.array([a.x, a.y, a.z], dtype=np.float64)


def restate(cam, w, h, model, offsets):
    """float64: (origin, direction, largest-magnitude operand of the sums) per set, each (h, w, 3)"""
    eye, hor, ver, corner = vec(cam.lookFrom), vec(cam.horizontal), vec(cam.vertical), vec(cam.cornerLowLeft)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for dx, dy in offsets.astype(np.float64):
        s, t = ((xs + dx) / w)[..., None], ((ys + dy) / h)[..., None]
        if model == abi.RAYS_EQUIRECT:
            phi, lat = float(F(6.2831855)) * (s - 0.5), float(F(3.1415927)) * (t - 0.5)
            d = np.concatenate([np.cos(lat) * np.cos(phi), np.sin(lat), np.cos(lat) * np.sin(phi)], axis=-1)
            yield np.broadcast_to(eye, d.shape), d, np.ones_like(d)
            continue
        P = corner + hor * s + ver * t
        big = np.maximum.reduce([np.abs(np.broadcast_to(corner, P.shape)), np.abs(hor * s), np.abs(ver * t), np.abs(P), np.abs(np.broadcast_to(eye, P.shape))])
        if model == abi.RAYS_ORTHOGRAPHIC:
            M = corner + hor * 0.5 + ver * 0.5
            big = np.maximum(big, np.maximum.reduce([np.abs(hor * 0.5), np.abs(ver * 0.5), np.abs(M)]))
            yield eye + (P - M), np.broadcast_to(M - eye, P.shape), big
        else:
            yield np.broadcast_to(eye, P.shape), P - eye, big


@pytest.mark.parametrize("model", (abi.RAYS_PINHOLE, abi.RAYS_ORTHOGRAPHIC, abi.RAYS_EQUIRECT), ids=("pinhole", "ortho", "equirect"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_generator_against_float64(size, model):
    w, h = size
    offsets = np.concatenate([np.zeros((1, 2), F), np.full((1, 2), 0.5, F), host.halton_offsets(5)[1:], np.array([[np.nextafter(F(1), F(0)), 0.0]], F)])
    for name, cam in cameras(w, h):
        got = host.generate_camera_rays(cam, w, h, model, len(offsets), offsets)
        assert got.shape == (len(offsets), h, w) and (got["tmax"] == FLT_MAX).all() and not got["_pad"].any()
        for k, (o, d, big) in enumerate(restate(cam, w, h, model, offsets)):
            tol = 1e-6 if model == abi.RAYS_EQUIRECT else 4.0 * np.spacing(big.astype(F)).astype(np.float64)
            eo, ed = np.abs(got[k]["origin"].astype(np.float64) - o), np.abs(got[k]["direction"].astype(np.float64) - d)
            print(f"{name} {w}x{h} model {model} set {k}: origin error / bound {np.max(eo / tol):.3f}, direction error / bound {np.max(ed / tol):.3f}")
            assert (eo <= tol).all() and (ed <= tol).all()
            if model == abi.RAYS_EQUIRECT:
                assert np.abs(np.linalg.norm(got[k]["direction"].astype(np.float64), axis=-1) - 1.0).max() < 2e-6


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pinhole_at_zero_offset_is_cast_rays_expression_bit_for_bit(size):
    w, h = size
    for name, cam in cameras(w, h):
        want = camera_rays(cam, w, h)                            # numpy binary32: castRay at lens radius 0 (conftest)
        for offsets in (None, np.zeros((1, 2), F)):
            got = host.generate_camera_rays(cam, w, h, abi.RAYS_PINHOLE, 1, offsets)[0].ravel()
            for field in ("origin", "direction", "tmax"):
                assert np.array_equal(np.ascontiguousarray(got[field]).view(np.uint32), np.ascontiguousarray(want[field]).view(np.uint32)), (name, field)


def to_binary32(q):
    """the fraction rounded once to binary32 (to nearest, ties to even)"""
    if q == 0:
        return F(0)
    e = 0
    while q * 2 ** e < 2 ** 23:
        e += 1
    n, r = divmod(q.numerator * 2 ** e, q.denominator)
    if 2 * r > q.denominator or (2 * r == q.denominator and n & 1):
        n += 1
    return np.ldexp(F(n), -e)


def radical_inverse(i, b):
    q, scale = Fraction(0), Fraction(1, b)
    while i:
        q += (i % b) * scale
        i //= b
        scale /= b
    return q


def test_halton_offsets_are_the_exact_fractions_rounded_once():
    n = 1500
    got = host.halton_offsets(n)
    assert got.shape == (n, 2) and got.dtype == F and (got >= 0).all() and (got < 1).all()
    want = np.array([[to_binary32(radical_inverse(k + 1, 2)), to_binary32(radical_inverse(k + 1, 3))] for k in range(n)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:3], np.array([[0.5, F(1) / F(3)], [0.25, F(2) / F(3)], [0.75, F(1) / F(9)]], F))
    assert host.halton_offsets(0).shape == (0, 2)


def test_argument_errors():
    cam = host.prepare_camera(8, 8)
    ok = dict(model=abi.RAYS_PINHOLE, n_sets=2, offsets=np.zeros((2, 2), F))
    assert host.generate_camera_rays(cam, 8, 8, **ok).shape == (2, 8, 8)
    for bad in (dict(n_sets=0, offsets=None), dict(n_sets=abi.TRC_MAX_RAY_SETS + 1, offsets=None), dict(model=3),
                dict(offsets=np.array([[0, 0], [1.0, 0]], F)), dict(offsets=np.array([[0, -0.5], [0, 0]], F)),
                dict(offsets=np.array([[np.nan, 0], [0, 0]], F)), dict(offsets=np.array([[0, 0], [0, np.inf]], F))):
        with pytest.raises(ValueError):
            host.generate_camera_rays(cam, 8, 8, **{**ok, **bad})
    L = host.lib()
    g = abi.RayGen(model=abi.RAYS_PINHOLE, n_sets=1)
    out = np.zeros(64 * 8, np.uint32)
    assert L.trc_host_generate_camera_rays(C.byref(cam), 8, 8, C.byref(g), out.ctypes.data) == abi.OK
    assert L.trc_host_generate_camera_rays(None, 8, 8, C.byref(g), out.ctypes.data) == abi.ERR_INVALID_ARG
    assert L.trc_host_generate_camera_rays(C.byref(cam), 8, 8, None, out.ctypes.data) == abi.ERR_INVALID_ARG
    assert L.trc_host_generate_camera_rays(C.byref(cam), 8, 8, C.byref(g), None) == abi.ERR_INVALID_ARG
    assert L.trc_host_generate_camera_rays(C.byref(cam), 0, 8, C.byref(g), out.ctypes.data) == abi.ERR_INVALID_ARG
    assert L.trc_host_generate_camera_rays(C.byref(cam), 8, 0, C.byref(g), out.ctypes.data) == abi.ERR_INVALID_ARG
