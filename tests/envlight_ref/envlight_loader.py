"""Wraps tests/envlight_ref/envlight_ref.cpp (the CPU restatement of TRC_FLAG_ENV_LIGHT's tables, sampler and pdf), which the oracle
library links in (oracle/Makefile)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Ref:
    def __init__(self, L):
        self.L = L

    def tables(self, rgb):
        """(h, w, 3) float32 map, rows bottom-up -> dict(weight (h, w), rows (h, w, 2), marg (h, 2), total)"""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        H, W = rgb.shape[:2]
        weight = np.empty((H, W), np.float32)
        rows = np.empty((H, W, 2), np.uint32)
        marg = np.empty((H, 2), np.uint32)
        total = C.c_double()
        self.L.envlight_ref_tables(rgb.ctypes.data, W, H, weight.ctypes.data, rows.ctypes.data, marg.ctypes.data, C.byref(total))
        return dict(weight=weight, rows=rows, marg=marg, total=total.value)

    def sample(self, t, draws):
        draws = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1, 6)
        H, W = t["weight"].shape
        out = np.empty((draws.shape[0], 4), np.float32)
        self.L.envlight_ref_sample(W, H, t["weight"].ctypes.data, t["rows"].ctypes.data, t["marg"].ctypes.data, t["total"],
                                   draws.ctypes.data, draws.shape[0], out.ctypes.data)
        return out

    def pdf(self, t, dirs):
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        H, W = t["weight"].shape
        out = np.empty(dirs.shape[0], np.float32)
        self.L.envlight_ref_pdf(W, H, t["weight"].ctypes.data, t["total"], dirs.ctypes.data, dirs.shape[0], out.ctypes.data)
        return out


def build():
    """the restatement as the oracle library holds it (oracle/Makefile links tests/envlight_ref/envlight_ref.cpp into liboracle.so: one CPU
    statement, one build of it).  make runs every time -- it does nothing when the library is newer than its sources -- so an edit of the
    restatement is never answered from a stale library; TRC_ORACLE_DIR names a build of somebody else's making (the sanitized one)."""
    if os.environ.get("TRC_ORACLE_DIR"):
        so = os.path.join(os.environ["TRC_ORACLE_DIR"], "liboracle.so")
    else:
        so = os.path.join(ROOT, "oracle", "liboracle.so")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(so)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.envlight_ref_tables.argtypes = [vp, u32, u32, vp, vp, vp, C.POINTER(C.c_double)]
    L.envlight_ref_sample.argtypes = [u32, u32, vp, vp, vp, C.c_double, vp, sz, vp]
    L.envlight_ref_pdf.argtypes = [u32, u32, vp, C.c_double, vp, sz, vp]
    L.envlight_ref_scale.argtypes = [u32, u32, C.c_double]
    L.envlight_ref_scale.restype = C.c_float
    return Ref(L)


def sun_sky(W, H, sun=(0.3, 0.7), sun_radius=0.03, sun_power=2000.0, sky=(0.4, 0.6, 1.0)):
    """a synthetic sun-and-sky map: a blue upper hemisphere fading to a dim ground and a small very bright disc at (u, w) = sun"""
    u = (np.arange(W, dtype=np.float64) + 0.5) / W
    w = (np.arange(H, dtype=np.float64) + 0.5) / H
    uu, ww = np.meshgrid(u, w)
    lat = np.pi * (ww - 0.5)
    up = np.clip(np.sin(lat), 0.0, 1.0)[..., None]
    img = 0.05 + up * np.array(sky)[None, None, :]
    phi, slat = 2 * np.pi * (uu - 0.5), lat
    d = np.stack([np.cos(slat) * np.cos(phi), np.sin(slat), np.cos(slat) * np.sin(phi)], -1)
    sp, sl = 2 * np.pi * (sun[0] - 0.5), np.pi * (sun[1] - 0.5)
    s = np.array([np.cos(sl) * np.cos(sp), np.sin(sl), np.cos(sl) * np.sin(sp)])
    img = img + (d @ s > np.cos(sun_radius))[..., None] * sun_power
    return np.ascontiguousarray(img, dtype=np.float32)
