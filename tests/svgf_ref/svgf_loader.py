"""Builds tests/svgf_ref/svgf_ref.cpp (the CPU restatement of the SVGF stage) into a directory of the caller's and wraps it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MISS = 0xFFFFFFFF
GBUF = np.dtype([("depth", np.float32), ("normal", np.float32, 3), ("albedo", np.float32, 3), ("id", np.uint32)])


class DenoiseParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("iterations", C.c_uint32), ("alpha_color", C.c_float), ("alpha_moments", C.c_float),
                ("sigma_z", C.c_float), ("normal_exponent", C.c_uint32), ("sigma_l", C.c_float), ("min_history", C.c_uint32)]


def params(demodulate=False, **kw):
    """the defaults of trc_denoise_default_params, then the named fields replaced"""
    p = DenoiseParams(1 if demodulate else 0, 5, 0.1, 0.2, 1.0, 128, 4.0, 4)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def build(out_dir):
    so = os.path.join(str(out_dir), "libsvgf_ref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "svgf_ref", "svgf_ref.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.svgf_ref_frame.argtypes = [C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.svgf_ref_frame.restype = C.c_int
    L.svgf_ref_normal_weight.argtypes = [C.c_float, C.c_uint32]
    L.svgf_ref_normal_weight.restype = C.c_float
    return Ref(L)


def cam_vectors(cam):
    """the 12 floats the filter reads from a trc_Camera: lookFrom, horizontal, vertical, cornerLowLeft"""
    f = lambda a: [a.x, a.y, a.z]
    return np.array(f(cam.lookFrom) + f(cam.horizontal) + f(cam.vertical) + f(cam.cornerLowLeft), dtype=np.float32)


class Ref:
    """One context's worth of state: frame() runs one trc_denoise on the CPU and keeps the history for the next."""

    def __init__(self, L):
        self.L = L
        self.reset()

    def reset(self):
        self.prev_cam = self.prev_g = self.hist_col = self.hist_mom = None

    def frame(self, p, cam, g, accum):
        H, W = g.shape
        cam = np.ascontiguousarray(cam, dtype=np.float32)
        g = np.ascontiguousarray(g)
        accum = np.ascontiguousarray(accum, dtype=np.float32)
        integ, hc, hm, out = (np.zeros((H, W, 4), np.float32) for _ in range(4))
        have = self.prev_cam is not None
        ptr = lambda a: a.ctypes.data if a is not None else None
        self.L.svgf_ref_frame(C.byref(p), W, H, cam.ctypes.data, ptr(self.prev_cam) if have else None, g.ctypes.data,
                              ptr(self.prev_g) if have else None, accum.ctypes.data, ptr(self.hist_col) if have else None,
                              ptr(self.hist_mom) if have else None, integ.ctypes.data, hc.ctypes.data, hm.ctypes.data, out.ctypes.data)
        self.prev_cam, self.prev_g, self.hist_col, self.hist_mom = cam, g, hc, hm
        return integ, hc, hm, out
