"""Builds tests/svgf_motion_ref/svgf_motion_ref.cpp (the CPU restatement of the SVGF stage with motion tracking) into a directory of
the caller's and wraps it, the way tests/svgf_ref/svgf_loader.py does for the stage without it (same compiler flags)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "svgf_ref"))
from svgf_loader import GBUF, MISS, DenoiseParams, cam_vectors, params  # noqa: E402,F401

MOTION = np.dtype([("prev", np.float32, 3), ("moved", np.uint32)])


def build(out_dir):
    so = os.path.join(str(out_dir), "libsvgf_motion_ref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "svgf_motion_ref", "svgf_motion_ref.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.svgf_motion_ref_frame.argtypes = [C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32] + [vp] * 12
    L.svgf_motion_ref_frame.restype = C.c_int
    return Ref(L)


class Ref:
    """One context's worth of state: frame() runs one trc_denoise on the CPU and keeps the history for the next."""

    def __init__(self, L):
        self.L = L
        self.reset()

    def reset(self):
        """what drops the history on the device: the next frame has no previous one"""
        self.prev_cam = self.prev_g = self.hist_col = self.hist_mom = None

    def frame(self, p, cam, g, accum, motion=None):
        """motion: (H, W) array of MOTION, or None for a trc_denoise with no snapshot in force (an all-zero plane)"""
        H, W = g.shape
        cam = np.ascontiguousarray(cam, dtype=np.float32)
        g = np.ascontiguousarray(g)
        accum = np.ascontiguousarray(accum, dtype=np.float32)
        if motion is not None:
            motion = np.ascontiguousarray(motion, dtype=MOTION)
            assert motion.shape == (H, W)
        integ, hc, hm, out = (np.zeros((H, W, 4), np.float32) for _ in range(4))
        have = self.prev_cam is not None
        ptr = lambda a: a.ctypes.data if a is not None else None
        self.L.svgf_motion_ref_frame(C.byref(p), W, H, cam.ctypes.data, ptr(self.prev_cam) if have else None, g.ctypes.data,
                                     ptr(self.prev_g) if have else None, ptr(motion), accum.ctypes.data,
                                     ptr(self.hist_col) if have else None, ptr(self.hist_mom) if have else None,
                                     integ.ctypes.data, hc.ctypes.data, hm.ctypes.data, out.ctypes.data)
        self.prev_cam, self.prev_g, self.hist_col, self.hist_mom = cam, g, hc, hm
        return integ, hc, hm, out
